// A batch of scatter reads on gfx950 in two launches and ONE pass over the
// bytes the reads take: preadv_probe_kernel, then unframe_scatter_batch_kernel
// (DESIGN.md section 22).
//
// preadv_probe_kernel is pread_probe_kernel (pread_batch_kernels.hip) with the
// entry's room given as the total of its fragments: one workgroup, thread e
// for entry e, probe_window (pread_batch_layout.h) with dst_cap = cap, the
// packet-count prefix over the regular entries by thread 0.  No arithmetic of
// its own.
//
// unframe_scatter_batch_kernel is unframe_window_batch_kernel with a scatter
// store: 16 waves a workgroup, the table image filled once behind the only
// barrier, workgroup b walks global packets g = b, b + G, ... found on the
// prefix array through the constant address space, wave v takes round v, two
// register sets take turns.  A packet's data is loaded and verified WHOLE
// (load_round, load_crcs, verify_round, the header and the ragged chunk by
// wave 0).  Only the bytes of the payload range [c_begin, w_end) are stored,
// payload position x at destination position y = x - c_begin of the entry's
// fragments (store_scatter, preadv_batch_lookup.h):
//   the round's cut to the window is empty      nothing is looked up or stored;
//   it is the whole round inside one fragment   store_round, the destination
//                                               inside that fragment: a read
//                                               into one fragment costs what
//                                               the pread batch costs;
//   otherwise                                   a scalar loop over the pieces
//     of the cut, one per fragment under it: a range over exactly the piece's
//     bytes, the lane pieces wholly inside as 16-B stores, the one or two that
//     hold its first or last byte without lying inside byte by byte.
// Which case a round is in, and every trip of the loop, is wave-uniform (the
// tables are read with scalar loads), and inside each case every lane issues
// the same vector-memory instructions: a lane with nothing to store uses an
// offset outside the range (kNowhere).  The fragment hint is the wave's own
// (Cursor), kept and reset by the rules of preadv_batch_lookup.h, consulted
// when a packet is STORED: the loads of the next packet, which may belong to
// another entry, are issued before.
//
// Any mismatch makes the lane that saw it store 1 into its entry's status
// word: a plain vector store, every writer the same value.  No atomics, no
// spinning, no cross-workgroup dependence.  The host hands a flagged entry to
// hdfs_crc32c_read_packets with its window and fragments, which overwrites
// what was stored.
//
// SAFETY.  Loads are the pread batch's: a packet's header, CRC and data regions
// lie inside [stream, stream + consumed), consumed <= len, by the probe's
// descriptor.  Stores: positions come from that descriptor, w_end - c_begin =
// read_len <= cap = at[nf] (probe_window's dst_cap test), so every cut lies in
// destination positions [0, at[nf]).  The fragment table comes from the ranges
// the host validated (device memory of one allocation each, clear of every
// stream and of each other), never from stream bytes.  Every store goes
// through a range_of descriptor over exactly one piece, and a piece lies inside
// one fragment: [base + foff, base + foff + (pe - ps)) with foff + (pe - ps) <=
// at[k + 1] - at[k] (next_piece).  The piece loop ends because the cut ends at
// or before at[nf], and it stops at a row that does not continue the one
// before.  The hardware drops what falls outside a range, so whatever the
// stream's bytes are, and whatever this file's offset arithmetic does, no
// stream content can move a store outside the fragments or the status array.
// Every write is a vector store; the tables are read through the constant
// address space.
#include "wire_fused_round.h"

#include "crc32c_frame.h"
#include "crc32c_outpkt.h"
#include "pread_batch_layout.h"
#include "preadv_batch_internal.h"
#include "preadv_batch_lookup.h"
#include "read_batch_header.h"
#include "read_batch_verify.h"
#include "wire_fused_batch_lookup.h"

namespace hdfs_preadv_batch {

using namespace hdfs_wire_fused;  // the round: Unit, range_of, load_round, store_round, crc::
using hdfs_pread_batch::kMaxTail;
using hdfs_pread_batch::PacketAt;
using hdfs_pread_batch::prefix_regular;
using hdfs_pread_batch::probe_window;
using hdfs_read_batch::crc_count;
using hdfs_read_batch::flag;
using hdfs_read_batch::load32;
using hdfs_read_batch::load_crcs;
using hdfs_read_batch::Round;
using hdfs_read_batch::verify_header;
using hdfs_read_batch::verify_round;
using hdfs_wirev_fused::AtOf;
using hdfs_wirev_fused::FragTab;

#ifndef CAS
#define CAS __attribute__((address_space(4)))
#endif

static_assert(kOutside == kNowhere, "the lookup header's offset outside every range is the round's");

constexpr uint32_t kExpectWords = 16;  // the expected header, 33 bytes at most; every lane reads a byte of it

// ---- the probe ----------------------------------------------------------------------
struct DeviceBytes {
  const uint8_t *s;
  __host__ __device__ const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

__global__ __launch_bounds__(1024) void preadv_probe_kernel(const Entry *__restrict__ in, uint32_t n, int proto,
                                                            uint32_t chunk_size, int ctype, uint32_t want_records,
                                                            uint64_t max_pkts, Window *__restrict__ desc,
                                                            uint32_t *__restrict__ slot,
                                                            uint32_t *__restrict__ status, uint32_t *__restrict__ pk0,
                                                            uint32_t *__restrict__ meta) {
  __shared__ uint32_t npk[kMaxEntries], at[kMaxEntries];
  const uint32_t e = threadIdx.x;
  Window w;
  bool regular = false;
  if (e < n) {
    const Entry x = in[e];
    regular = probe_window(DeviceBytes{x.stream}, x.len, x.dst_cap, x.client_offset, x.read_len, proto, chunk_size,
                           ctype, want_records != 0u, max_pkts, w);
    w.d.stream = x.stream;
    w.d.dst = nullptr;
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
// destination of payload position x is position x - cb of the entry's
// fragments.
struct WRound {
  Round r;
  uint64_t pos0;         // the packet's first data byte
  uint64_t cb, we;       // the window
  uint32_t slot, entry;  // the cursor's key; the fragments' (fr0)
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
  u.dst = 0u;
  r.out0 = 0u;
  wr.cb = w->c_begin;
  wr.we = w->w_end;
  wr.pos0 = doff;
  wr.slot = k;
  wr.entry = p->entry;
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

// The fragment table of a call, through the constant address space.
struct FragTables {
  const CAS uint32_t *fr0;
  FragTab ft;
};

// Lane piece q of the round, held by the lane whose lo is 16 q mod 1024 in
// register set q / 64, stored byte by byte where it lies in the piece [ps, pe)
// (rg: the range of exactly the piece).  Every lane issues the sixteen stores;
// all but the owner's bytes inside go nowhere.
FUSED_DEV void store_edge(__amdgpu_buffer_rsrc_t rg, const u32x4 (&v)[4], uint32_t q, uint32_t ps, uint32_t pe,
                          uint32_t lo) {
  const uint32_t o = 16u * q, kq = o >> 10;
  const bool mine = lo == (o & 1023u);
  const u32x4 x = kq == 0u ? v[0] : kq == 1u ? v[1] : kq == 2u ? v[2] : v[3];  // uniform
#pragma unroll
  for (uint32_t j = 0; j < 16; j++)
    store8(rg, mine ? byte_at(o + j, ps, pe) : kNowhere, (x[j >> 2] >> (8u * (j & 3u))) & 0xFFu);
}

// The round's full chunks, from the registers of its loads, over the entry's
// fragments.
FUSED_DEV void store_scatter(const u32x4 (&v)[4], const WRound &wr, const FragTables &ftab, Cursor &c, uint32_t wave,
                             uint32_t lo) {
  const Unit &u = wr.r.u;
  const uint32_t n = u.nfr * kChunk;
  const uint64_t x0 = wr.pos0 + uint64_t(kRound) * wave;
  uint32_t bytes;
  const uint64_t a = window_cut(wr, x0, n, bytes);
  if (bytes == 0u) return;  // uniform (rule 4)
  seek_slot(c, wr.slot);
  const Slice s = slice_of(ftab.fr0, wr.entry);
  const FragTab t = ftab.ft + s.first;
  const uint64_t y0 = a - wr.cb;
  const uint32_t k = seek_frag(AtOf{t}, s.nf, y0, c);
  const uint32_t sa = uint32_t(a - x0), sb = sa + bytes;
  if (unseamed(AtOf{t}, k, y0, sa, sb, n)) {  // uniform: the pread batch's store, inside fragment k
    Unit su = u;
    su.dst = reinterpret_cast<uintptr_t>(t[k].base) + uintptr_t(y0 - t[k].at);
    store_round(v, su, lo);
    return;
  }
  Walk w{k, sa};
  Piece p;
  while (next_piece(AtOf{t}, s.nf, y0, sa, sb, w, p)) {  // uniform
    const __amdgpu_buffer_rsrc_t rg =
        range_of(reinterpret_cast<uintptr_t>(t[p.k].base) + uintptr_t(p.foff), p.pe - p.ps);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) store16(rg, whole_at(lo + 1024u * j, p.ps, p.pe), v[j]);
    uint32_t q;
    if (head_edge(p.ps, p.pe, q)) store_edge(rg, v, q, p.ps, p.pe, lo);
    if (tail_edge(p.ps, p.pe, q)) store_edge(rg, v, q, p.ps, p.pe, lo);
  }
}

// The packet's chunk shorter than 512 B (n bytes behind its full chunks, n =
// 0: none), by one whole wave: the pread batch's verify_ragged with the byte
// stores clipped piece by piece.  Frame byte f holds chunk byte f - pad,
// payload position x0 + f - pad; a piece's range starts at chunk byte ps.
FUSED_DEV bool verify_ragged(const uint32_t *img, const uint32_t *tab, const WRound &wr, const FragTables &ftab,
                             Cursor &c, uint32_t lane) {
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
  if (bytes != 0u) {  // uniform (rule 4)
    seek_slot(c, wr.slot);
    const Slice s = slice_of(ftab.fr0, wr.entry);
    const FragTab t = ftab.ft + s.first;
    const uint64_t y0 = a - wr.cb;
    const uint32_t sa = uint32_t(a - x0), sb = sa + bytes;
    Walk w{seek_frag(AtOf{t}, s.nf, y0, c), sa};
    Piece p;
    while (next_piece(AtOf{t}, s.nf, y0, sa, sb, w, p)) {  // uniform
      const __amdgpu_buffer_rsrc_t rd =
          range_of(reinterpret_cast<uintptr_t>(t[p.k].base) + uintptr_t(p.foff), p.pe - p.ps);
      const uint32_t skip = pad + p.ps;  // <= 1024: below it the offset wraps out of the range
#pragma unroll
      for (uint32_t j = 0; j < 8; j++) store8(rd, 8u * lane + j - skip, b[j]);
    }
  }
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

__global__ __launch_bounds__(1024) void unframe_scatter_batch_kernel(const CAS Window *dt, const CAS uint32_t *pk0,
                                                                     const CAS uint32_t *meta,
                                                                     const CAS uint32_t *fr0, FragTab ft,
                                                                     uint32_t *status, uint32_t proto,
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
  const FragTables ftab{fr0, ft};
  Cursor c;  // the wave's fragment hint, of the packet being stored
  uint32_t g = blockIdx.x, k = 0u;
  // Two register sets take turns, as in unframe_window_batch_kernel.
  u32x4 ra[4], rb[4];
  uint32_t wa, wb;
  WRound r = round_at(dt, pk0, st, nw, total, g, k, wave);
  load_round(ra, r.r.u, lo);
  wa = load_crcs(r.r.u, wave, lane);
  auto step = [&](const u32x4(&cur)[4], uint32_t wcur, u32x4(&nxt)[4], uint32_t &wnxt) {
    const WRound rn = round_at(dt, pk0, st, nw, total, g + G, k, wave);  // g + G < 2^32: total < 2^29, G <= 1024
    load_round(nxt, rn.r.u, lo);  // the next packet's loads, ahead of this round's stores
    wnxt = load_crcs(rn.r.u, wave, lane);
    store_scatter(cur, r, ftab, c, wave, lo);
    bool bad = verify_round(lds, cur, wcur, r.r.u, lane, init512);
    if (wave == 0u) {
      bad |= verify_header(hdr, proto, r.r, lane);
      bad |= verify_ragged(lds, tab, r, ftab, c, lane);
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

hipError_t prepare_unframe_scatter_batch() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&unframe_scatter_batch_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kExpectWords) * sizeof(uint32_t)));
}

hipError_t launch_probe(void *tables, uint32_t n, uint32_t nfe, int proto, uint32_t chunk_size, int ctype,
                        bool want_records, uint64_t max_pkts, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries) return hipErrorInvalidValue;
  const Tables t(n, nfe);
  uint8_t *b = static_cast<uint8_t *>(tables) + t.base;
  hipLaunchKernelGGL(preadv_probe_kernel, dim3(1), dim3(kMaxEntries), 0, stream,
                     reinterpret_cast<const Entry *>(b + t.p.in), n, proto, chunk_size, ctype,
                     want_records ? 1u : 0u, max_pkts, reinterpret_cast<Window *>(b + t.p.desc),
                     reinterpret_cast<uint32_t *>(b + t.p.slot), reinterpret_cast<uint32_t *>(b + t.p.status),
                     reinterpret_cast<uint32_t *>(b + t.p.pk0), reinterpret_cast<uint32_t *>(b + t.p.meta));
  return hipGetLastError();
}

hipError_t launch_unframe_scatter_batch(void *tables, uint32_t n, uint32_t nfe, uint32_t proto,
                                        const uint32_t *crc_tab, uint32_t groups, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !nfe || !groups || groups > kBatchMaxGroups || !crc_tab)
    return hipErrorInvalidValue;
  const Tables t(n, nfe);
  uint8_t *f = static_cast<uint8_t *>(tables), *b = f + t.base;
  hipLaunchKernelGGL(unframe_scatter_batch_kernel, dim3(groups), dim3(64 * kWaves),
                     (crc::kImageWords + kExpectWords) * sizeof(uint32_t), stream, (const CAS Window *)(b + t.p.desc),
                     (const CAS uint32_t *)(b + t.p.pk0), (const CAS uint32_t *)(b + t.p.meta),
                     (const CAS uint32_t *)(f + t.fr0), (FragTab)(f + t.ft),
                     reinterpret_cast<uint32_t *>(b + t.p.status), proto, crc_tab);
  return hipGetLastError();
}

}  // namespace hdfs_preadv_batch
