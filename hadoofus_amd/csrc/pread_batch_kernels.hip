// A batch of positional reads on gfx950 in two launches and ONE pass over the
// bytes the reads take: pread_probe_kernel, then unframe_window_batch_kernel
// (DESIGN.md section 21).
//
// pread_probe_kernel is one workgroup, thread e for entry e.  It runs
// probe_window (pread_batch_layout.h: probe_entry's framing of packet 0 and
// the tail, then the window arithmetic, all of it run on host streams by the
// CPU suite) and cuts the entry to the m packets its read takes.  Thread 0
// lays the packet-count prefix over the regular entries (prefix_regular) from
// those m, not from the streams' packet counts: a 64 KiB window in a 128 MiB
// stream costs the main launch one or two packets.
//
// unframe_window_batch_kernel is unframe_fused_batch_kernel
// (read_batch_kernels.hip) with a windowed store: 16 waves a workgroup, the
// table image filled once behind the only barrier, workgroup b walks global
// packets g = b, b + G, ... found with write_of on the prefix array through
// the constant address space, wave v takes round v, two register sets take
// turns.  A packet's data is loaded and verified WHOLE (load_round, load_crcs,
// verify_round, the header and the ragged chunk by wave 0): a corrupt chunk in
// the skipped head of packet 0 or behind the read's end in packet m - 1 flags
// the entry like any other.  Only the bytes of the payload range [c_begin,
// w_end) are stored, payload position x at dst + (x - c_begin)
// (store_window):
//   a round wholly inside the window    store_round, as in the read batch;
//   a round wholly outside              store_round over an empty range;
//   a round that crosses an edge (at most two an entry): its 16-B pieces that
//     lie wholly inside as 16-B stores, the one or two pieces that straddle an
//     edge byte by byte, all through a range_of descriptor over exactly the
//     bytes of the intersection.
// Which case a round is in is wave-uniform (a scalar branch), and inside each
// case every lane issues the same vector-memory instructions: a lane with
// nothing to store uses an offset outside the range (kNowhere), as flag and
// load_crcs do.  The waves of a workgroup do NOT all issue one instruction
// sequence, though: a wave whose round crosses an edge issues four 16-B and 32
// one-byte stores more than its neighbours (store_window's branch), as wave 0
// alone issues the header's and the ragged chunk's accesses.  Inside a wave
// control flow stays uniform, which is what the compiler's counted waits need.
//
// Any mismatch makes the lane that saw it store 1 into its entry's status
// word: a plain vector store, every writer the same value.  No atomics, no
// spinning, no cross-workgroup dependence.  The host hands a flagged entry to
// hdfs_crc32c_read_packets with its window, which overwrites its destination.
//
// SAFETY.  Every address of the main launch comes from the probe's descriptor.
// Loads: a packet's header, CRC and data regions lie at stream_off + [0, hb +
// 4 ncrc + dlen) with every packet of the m inside [0, consumed), consumed <=
// len (probe_entry validated the whole stream's chain from the lengths alone,
// and the cut keeps a prefix of it).  Stores: a round's or a ragged chunk's
// range is the intersection of its payload bytes with [c_begin, w_end),
// shifted by -c_begin: inside [dst, dst + read_len), read_len <= dst_cap.
// Every vector access goes through range_of over exactly those bytes and the
// hardware drops what falls outside, so whatever the stream's bytes are, and
// whatever this file's offset arithmetic does, no load leaves [stream, stream
// + len) and no store leaves [dst, dst + min(dst_cap, read_len)) or the status
// array.  The host checked that every range lies inside one device allocation
// and that no destination overlaps a stream or another destination.
#include "crc32c_frame.h"
#include "crc32c_outpkt.h"
#include "pread_batch_internal.h"
#include "pread_batch_layout.h"
#include "read_batch_verify.h"
#include "wire_fused_batch_lookup.h"
#include "wire_fused_round.h"

namespace hdfs_pread_batch {

using namespace hdfs_wire_fused;  // the round: Unit, range_of, load_round, store_round, crc::
using hdfs_read_batch::crc_count;
using hdfs_read_batch::flag;
using hdfs_read_batch::has_sync;
using hdfs_read_batch::load32;
using hdfs_read_batch::load_crcs;
using hdfs_read_batch::Round;
using hdfs_read_batch::verify_round;

#define CAS __attribute__((address_space(4)))

constexpr uint32_t kExpectWords = 16;  // the expected header, 33 bytes at most; every lane reads a byte of it

// ---- the probe ----------------------------------------------------------------------
struct DeviceBytes {
  const uint8_t *s;
  __host__ __device__ const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

__global__ __launch_bounds__(1024) void pread_probe_kernel(const Entry *__restrict__ in, uint32_t n, int proto,
                                                           uint32_t chunk_size, int ctype, uint32_t want_records,
                                                           uint64_t max_pkts, Window *__restrict__ desc,
                                                           uint32_t *__restrict__ slot, uint32_t *__restrict__ status,
                                                           uint32_t *__restrict__ pk0, uint32_t *__restrict__ meta) {
  __shared__ uint32_t npk[kMaxEntries], at[kMaxEntries];
  const uint32_t e = threadIdx.x;
  Window w;
  bool regular = false;
  if (e < n) {
    const Entry x = in[e];
    regular = probe_window(DeviceBytes{x.stream}, x.len, x.dst_cap, x.client_offset, x.read_len, proto, chunk_size,
                           ctype, want_records != 0u, max_pkts, w);
    w.d.stream = x.stream;
    w.d.dst = x.dst;
    w.d.entry = e;
  }
  npk[e] = regular ? w.d.npk : 0u;  // the packets the read takes, not the stream's
  __syncthreads();
  if (e == 0u) {
    const uint32_t nreg = prefix_regular(npk, n, at, pk0);
    meta[0] = nreg;
    meta[1] = pk0[nreg];
  }
  __syncthreads();
  if (e < n) {
    const uint32_t s = at[e];
    slot[e] = s;
    if (s != kNoSlot) {
      desc[s] = w;
      status[s] = 0u;
    }
  }
}

// ---- the main launch ------------------------------------------------------------------
// The wave's round of a packet (read_batch_verify.h) and its place in the
// window, in payload positions.  r.out0 and r.u.dst are not used here: the
// destination of payload position x is wdst + x.
struct WRound {
  Round r;
  uintptr_t wdst;       // the entry's dst - c_begin
  uint64_t pos0;        // the packet's first data byte
  uint64_t cb, we;      // the window
};

FUSED_DEV WRound round_at(const CAS Window *tab, const CAS uint32_t *pk0, uintptr_t status, uint32_t nw,
                          uint32_t total, uint32_t g, uint32_t &k, uint32_t wave) {
  const bool in = g < total;
  if (in) k = write_of(pk0, nw, g, k);
  const CAS Window *w = tab + k;
  const CAS Desc *p = &w->d;
  const uint32_t i = in ? g - pk0[k] : 0u, nbody = p->nbody;
  const bool body = i < nbody;
  const CAS PacketAt *t = p->tail + (body ? 0u : (i - nbody < kMaxTail ? i - nbody : 0u));  // i - nbody < ntail
  const uint32_t dlen0 = p->dlen0;
  const uint64_t soff = body ? uint64_t(i) * p->stride : t->stream_off;
  const uint64_t doff = body ? uint64_t(i) * dlen0 : t->dst_off;
  WRound wr;
  Round &r = wr.r;
  Unit &u = r.u;
  u.p.wire_off = soff;
  u.p.data_off = doff;
  u.p.off = body ? p->off0 + int64_t(uint64_t(i) * dlen0) : t->off;
  u.p.seq = body ? p->seq0 + int64_t(i) : t->seq;
  u.p.dlen = in ? (body ? dlen0 : t->dlen) : 0u;
  u.p.ncrc = crc_count(u.p.dlen);
  u.p.cidx = 0u;
  u.p.last = body ? p->last0 : t->last;
  r.sync = body ? p->sync0 : t->sync;
  u.hb = in ? (body ? p->hb0 : t->hb) : 0u;
  u.h0 = reinterpret_cast<uintptr_t>(p->stream) + soff;
  u.c0 = u.h0 + u.hb;
  u.d0 = u.c0 + 4u * uintptr_t(u.p.ncrc);
  const uint32_t nfull = u.p.dlen / kChunk, first = kRoundChunks * wave;
  u.nfr = nfull > first ? (nfull - first < kRoundChunks ? nfull - first : kRoundChunks) : 0u;
  u.src = u.d0 + uintptr_t(kRound) * wave;
  wr.cb = w->c_begin;
  wr.we = w->w_end;
  wr.pos0 = doff;
  wr.wdst = reinterpret_cast<uintptr_t>(p->dst) - uintptr_t(wr.cb);
  r.out0 = wr.wdst + uintptr_t(doff);
  u.dst = r.out0 + uintptr_t(kRound) * wave;
  r.status = status + 4u * uintptr_t(k);
  return wr;
}

// The payload bytes [x0, x0 + n) cut to the window: [a, a + *bytes), *bytes = 0
// when they miss it.  Uniform.
FUSED_DEV uint64_t window_cut(const WRound &wr, uint64_t x0, uint32_t n, uint32_t &bytes) {
  const uint64_t x1 = x0 + n, a = x0 > wr.cb ? x0 : wr.cb, b = x1 < wr.we ? x1 : wr.we;
  bytes = b > a ? uint32_t(b - a) : 0u;
  return a;
}

// Piece q of the round (its bytes [16 q, 16 q + 16)), held by the lane whose lo
// is 16 q mod 1024 in register set q / 64, stored byte by byte where it lies
// in [sa, sb).  Every lane issues the sixteen stores; all but the owner's
// bytes inside go nowhere.
FUSED_DEV void store_edge(__amdgpu_buffer_rsrc_t rg, const u32x4 (&v)[4], uint32_t q, bool on, uint32_t sa,
                          uint32_t sb, uint32_t lo) {
  const uint32_t o = 16u * q, kq = o >> 10;
  const bool mine = on && lo == (o & 1023u);
  const u32x4 x = kq == 0u ? v[0] : kq == 1u ? v[1] : kq == 2u ? v[2] : v[3];  // uniform
#pragma unroll
  for (uint32_t j = 0; j < 16; j++) {
    const uint32_t at = o + j;
    store8(rg, mine && at >= sa && at < sb ? at - sa : kNowhere, (x[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
  }
}

// The round's full chunks, from the registers of its loads, to the window.
FUSED_DEV void store_window(const u32x4 (&v)[4], const WRound &wr, uint32_t wave, uint32_t lo) {
  const Unit &u = wr.r.u;
  const uint32_t n = u.nfr * kChunk;
  const uint64_t x0 = wr.pos0 + uint64_t(kRound) * wave;
  uint32_t bytes;
  const uint64_t a = window_cut(wr, x0, n, bytes);
  const bool whole = bytes == n;  // (n == 0: a round of nothing)
  Unit su = u;
  su.nfr = whole ? u.nfr : 0u;    // outside, or crossing: an empty range
  store_round(v, su, lo);
  if (bytes != 0u && !whole) {  // uniform: the round crosses the window's start or its end, or both
    const uint32_t sa = uint32_t(a - x0), sb = sa + bytes;
    const __amdgpu_buffer_rsrc_t rg = range_of(wr.wdst + uintptr_t(a), bytes);
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t o = lo + 1024u * k;
      store16(rg, o >= sa && o + 16u <= sb ? o - sa : kNowhere, v[k]);
    }
    const uint32_t qa = sa >> 4, qb = (sb - 1u) >> 4;
    store_edge(rg, v, qa, (sa & 15u) != 0u || 16u * qa + 16u > sb, sa, sb, lo);
    store_edge(rg, v, qb, qb != qa && (sb & 15u) != 0u, sa, sb, lo);
  }
}

// read_batch_kernels.hip's verify_header, restated: tests/test_read_batch_cpu.py
// keeps that file's text (put_out_header among it) where it is, so the
// function cannot move to read_batch_verify.h.  The packet's header, by one
// whole wave: lane 0 composes the expected one into LDS, lane t compares byte
// t with the stream's.
FUSED_DEV bool verify_header(uint32_t *hdr, uint32_t proto, const Round &r, uint32_t lane) {
  const Unit &u = r.u;
  if (lane == 0u) {
    uint8_t *p = reinterpret_cast<uint8_t *>(hdr);
    uint8_t *e = hdfs_crc32c::outpkt::put_out_header(p, int(proto), u.p.off, u.p.seq, u.p.last != 0u,
                                                     int32_t(u.p.dlen), u.p.ncrc);
    if (has_sync(int(proto), u.hb)) {  // hlen 27: syncBlock behind the required fields
      p[5] = uint8_t(hdfs_crc32c::outpkt::kHdrProtoBytes + 2u);
      e[0] = 0x28;
      e[1] = r.sync ? 1 : 0;
    }
  }
  // a wave's LDS operations execute in order; the fences keep the compiler from reordering them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t want = reinterpret_cast<const uint8_t *>(hdr)[lane];
  const uint32_t got = load8(range_of(u.h0, u.hb), lane) & 0xFFu;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return lane < u.hb && got != want;
}

// The packet's chunk shorter than 512 B (n bytes behind its full chunks, n =
// 0: none), by one whole wave: the read batch's verify_ragged with the byte
// stores clipped to the window.  Frame byte f holds chunk byte f - pad, payload
// position x0 + f - pad; the range starts at payload position a >= x0.
FUSED_DEV bool verify_ragged(const uint32_t *img, const uint32_t *tab, const WRound &wr, uint32_t lane) {
  const Unit &u = wr.r.u;
  const uint32_t nfull = u.p.dlen / kChunk, n = u.p.dlen % kChunk, pad = kChunk - n;
  const __amdgpu_buffer_rsrc_t rs = range_of(u.d0 + uintptr_t(kChunk) * nfull, n);
  const uint32_t wire = load32(range_of(u.c0 + 4u * uintptr_t(nfull), n ? 4u : 0u), lane == 0u ? 0u : kNowhere);
  uint32_t b[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) b[j] = load8(rs, 8u * lane + j - pad) & 0xFFu;
  const uint64_t x0 = wr.pos0 + uint64_t(kChunk) * nfull;
  uint32_t bytes;
  const uint64_t a = window_cut(wr, x0, n, bytes);
  const uint32_t skip = pad + (bytes ? uint32_t(a - x0) : 0u);  // <= 1024: below it the offset wraps out of the range
  const __amdgpu_buffer_rsrc_t rd = range_of(wr.wdst + uintptr_t(a), bytes);
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) store8(rd, 8u * lane + j - skip, b[j]);
  uint32_t val = 0u;
  if (n) {  // uniform; no vector-memory access inside but the constant's scalar load
    const uint32_t w0 = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    const uint32_t w1 = b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24);
    const uint32_t i = lane & 7u;  // the lane's piece: frame bytes [64 i, 64 i + 64), held by lanes 8i .. 8i + 7
    uint32_t x[16];
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
      const int from = int(4u * (8u * i + j));
      x[2 * j] = uint32_t(__builtin_amdgcn_ds_bpermute(from, int(w0)));
      x[2 * j + 1] = uint32_t(__builtin_amdgcn_ds_bpermute(from, int(w1)));
    }
    val = crc::chunk_final(fold8(crc::piece_shift(img, i, crc::piece_raw(img, lane, x))), tab[crc::kCompactInit + n]);
  }
  return lane == 0u && n != 0u && wire != val;
}

__global__ __launch_bounds__(1024) void unframe_window_batch_kernel(const CAS Window *dt, const CAS uint32_t *pk0,
                                                                    const CAS uint32_t *meta, uint32_t *status,
                                                                    uint32_t proto,
                                                                    const uint32_t *__restrict__ tab) {
  extern __shared__ uint32_t lds[];
  const uint32_t nw = meta[0], total = meta[1];
  if (blockIdx.x >= total) return;  // uniform: no packet for this workgroup (so nw >= 1 below)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  uint32_t *hdr = lds + crc::kImageWords;
  fill_image(lds, tab, tid);
  const uint32_t init512 = tab[crc::kCompactInit + kChunk];
  __syncthreads();
  const uint32_t lo = 64u * (lane & 15u) + 16u * (lane >> 4);
  const uint32_t G = gridDim.x;
  const uintptr_t st = reinterpret_cast<uintptr_t>(status);
  uint32_t g = blockIdx.x, k = 0u;
  // Two register sets take turns, as in unframe_fused_batch_kernel.
  u32x4 ra[4], rb[4];
  uint32_t wa, wb;
  WRound r = round_at(dt, pk0, st, nw, total, g, k, wave);
  load_round(ra, r.r.u, lo);
  wa = load_crcs(r.r.u, wave, lane);
  auto step = [&](const u32x4(&cur)[4], uint32_t wcur, u32x4(&nxt)[4], uint32_t &wnxt) {
    const WRound rn = round_at(dt, pk0, st, nw, total, g + G, k, wave);  // g + G < 2^32: total < 2^29, G <= 1024
    load_round(nxt, rn.r.u, lo);  // the next packet's loads, ahead of this round's stores
    wnxt = load_crcs(rn.r.u, wave, lane);
    store_window(cur, r, wave, lo);
    bool bad = verify_round(lds, cur, wcur, r.r.u, lane, init512);
    if (wave == 0u) {
      bad |= verify_header(hdr, proto, r.r, lane);
      bad |= verify_ragged(lds, tab, r, lane);
    }
    flag(r.r, bad);
    g += G;
    r = rn;
  };
  while (g < total) {
    step(ra, wa, rb, wb);
    if (g >= total) break;
    step(rb, wb, ra, wa);
  }
}

hipError_t prepare_unframe_window_batch() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&unframe_window_batch_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kExpectWords) * sizeof(uint32_t)));
}

hipError_t launch_probe(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype, bool want_records,
                        uint64_t max_pkts, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(pread_probe_kernel, dim3(1), dim3(kMaxEntries), 0, stream,
                     reinterpret_cast<const Entry *>(b + t.in), n, proto, chunk_size, ctype, want_records ? 1u : 0u,
                     max_pkts, reinterpret_cast<Window *>(b + t.desc), reinterpret_cast<uint32_t *>(b + t.slot),
                     reinterpret_cast<uint32_t *>(b + t.status), reinterpret_cast<uint32_t *>(b + t.pk0),
                     reinterpret_cast<uint32_t *>(b + t.meta));
  return hipGetLastError();
}

hipError_t launch_unframe_window_batch(void *tables, uint32_t n, uint32_t proto, const uint32_t *crc_tab,
                                       uint32_t groups, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !groups || groups > kBatchMaxGroups || !crc_tab)
    return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(unframe_window_batch_kernel, dim3(groups), dim3(64 * kWaves),
                     (crc::kImageWords + kExpectWords) * sizeof(uint32_t), stream, (const CAS Window *)(b + t.desc),
                     (const CAS uint32_t *)(b + t.pk0), (const CAS uint32_t *)(b + t.meta),
                     reinterpret_cast<uint32_t *>(b + t.status), proto, crc_tab);
  return hipGetLastError();
}

}  // namespace hdfs_pread_batch
