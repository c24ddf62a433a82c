// A batch of verified reads re-framed as writes on gfx950 in two launches and
// ONE pass over the bytes: probe_relay_kernel, then relay_fused_batch_kernel
// (DESIGN.md section 25).
//
// probe_relay_kernel is one workgroup, thread e for entry e.  It runs the read
// batch's probe_entry as it stands (read_batch_layout.h; no destination limit,
// no records) on the entry's input stream, and for a regular one writes the
// output side of the descriptor: the write's packet count and stream length
// (out_shape, relay_batch_lookup.h).  An entry takes the kernel when its input
// is regular, consumed is below 4 GiB, the write starts on the chunk grid and
// its stream fits wire_cap.  Thread 0 lays the packet-count prefix over the
// OUTPUT packets of those entries (prefix_regular); the others get no slot and
// the main launch never touches them.
//
// relay_fused_batch_kernel has frame_fused_batch_kernel's organisation
// (wire_fused_batch_kernels.hip) and its round (wire_fused_round.h): a
// workgroup is 16 waves, the table image is filled once per workgroup behind
// the only barrier, workgroup b walks global output packets g = b, b + G, ...,
// found with write_of (wire_fused_batch_lookup.h) on the prefix array through
// the constant address space.  Wave v takes round v (4 KiB, eight chunks) of
// the output packet.  The round's registers -- load_round's -- are filled from
// the INPUT stream: each of the eight chunks from the place relay_batch_lookup.h
// gives it (the round may span several input packets; every seam lies between
// two chunks, so a lane's 16-byte piece never straddles one), and lane 8c loads
// chunk c's four CRC bytes from their place there.  store_round stores the
// registers into the output packet's data region, verify_round
// (read_batch_verify.h) runs the lane arithmetic once and compares chunk c's
// CRC with the loaded word, and lane 8c stores that word into the output
// packet's CRC region: where the comparison holds it is the CRC of the bytes
// just stored, where it does not the entry is flagged and rewritten.  Wave 0
// composes and stores the output header (header) and takes the chunk shorter
// than 512 B: load, store, CRC, comparison, CRC store.  The input headers an
// output packet answers for (first_header, end_header) are dealt over the 16
// waves and compared with the predicted ones (read_batch_header.h's
// verify_header).  Two register sets take turns, and the next packet's loads
// are issued ahead of the current round's stores.
//
// Any mismatch makes the lane that saw it store 1 into its entry's status word
// (flag): a plain vector store, every writer the same value.  No atomics, no
// spinning, no dependence between workgroups.  The host serves a flagged entry
// again, through hdfs_crc32c_read_packets and the fused framing kernel.
//
// INVARIANTS.  Every address of the main launch comes from the probe's
// descriptor and the host-validated entry, never from stream bytes: the probe
// validated nbody * stride + tail == consumed <= len from the lengths alone,
// and wire_len <= wire_cap.  Every vector access goes through range_of over
// exactly the bytes it may touch: one range over [stream, stream + consumed)
// for a round's seamed loads and its CRC words (empty when the round holds no
// full chunk; a lane or a chunk with nothing to load reads offset 0 of it, so no
// offset relies on lying outside a range of up to 4 GiB), exact ranges for an
// input header, for the ragged chunk and its CRC word in the input, for an
// output packet's header, CRC words, data round and ragged chunk, and for the
// entry's status word.  So whatever the stream's bytes are, and they may change
// under the kernel, no load leaves [stream, stream + len) and no store leaves
// [wire, wire + wire_len) or the status array: a corrupt stream costs a
// fallback, never an access out of range.  All writes are vector stores.  The
// probe's own loads are frame_step's.  The host checked that every range lies
// inside one device allocation and that no wire range overlaps a stream or
// another wire range, so no byte a wave loads is one another wave stores.
//
// hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S: see DESIGN.md section
// 25 for the register counts; private_segment_fixed_size 0 and
// group_segment_fixed_size 0 (dynamic LDS only: the table image and 64 bytes of
// expected header per wave) in the main kernel, no flat_ or scratch_
// instruction.
#include "crc32c_frame.h"
#include "crc32c_outpkt.h"
#include "read_batch_header.h"
#include "read_batch_layout.h"
#include "read_batch_verify.h"
#include "relay_batch_internal.h"
#include "relay_batch_lookup.h"
#include "wire_fused_batch_lookup.h"
#include "wire_fused_round.h"

namespace hdfs_relay_batch {

using namespace hdfs_read_batch;  // the read side: probe_entry, Round, verify_round, verify_header, flag; the round

#define CAS __attribute__((address_space(4)))

constexpr uint32_t kExpectWords = 16;  // a header, 33 bytes at most, per wave; every lane reads a byte of it

// ---- the probe ----------------------------------------------------------------------
struct DeviceBytes {
  const uint8_t *s;
  __host__ __device__ const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

__global__ __launch_bounds__(1024) void probe_relay_kernel(const hdfs_relay_batch::Entry *__restrict__ in, uint32_t n,
                                                           int proto, uint32_t chunk_size, int ctype,
                                                           hdfs_relay_batch::Desc *__restrict__ desc,
                                                           uint32_t *__restrict__ slot, uint32_t *__restrict__ status,
                                                           uint32_t *__restrict__ pk0, uint32_t *__restrict__ meta) {
  __shared__ uint32_t npk[kMaxEntries], at[kMaxEntries];
  const uint32_t e = threadIdx.x;
  hdfs_relay_batch::Desc d;
  bool takes = false;
  if (e < n) {
    const hdfs_relay_batch::Entry x = in[e];
    takes = probe_entry(DeviceBytes{x.stream}, x.len, ~uint64_t(0), proto, chunk_size, ctype, false, 0, d.in);
    d.in.stream = x.stream;
    d.in.dst = nullptr;
    d.in.entry = e;
    uint64_t wire_len = 0, out_npk = 0;
    if (takes) {
      d.g = geom_of(d.in);
      out_shape(d.in.delivered, x.hb, x.finish != 0u, wire_len, out_npk);
      takes = d.in.consumed < kMaxConsumed && (uint64_t(x.off) % kGrid) == 0u && wire_len <= x.wire_cap &&
              out_npk <= kMaxPackets;
    }
    d.wire = x.wire;
    d.wire_len = wire_len;
    d.off = x.off;
    d.seq = x.seq;
    d.npk = uint32_t(out_npk);
    d.hb = x.hb;
    d.finish = x.finish;
    d.pad = 0u;
  }
  npk[e] = takes ? d.npk : 0u;
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
      desc[s] = d;
      status[s] = 0u;
    }
  }
}

// ---- the main launch ------------------------------------------------------------------
// The wave's round of a global output packet.  r.u: the OUTPUT packet's regions
// and the round's place there (unit_of; u.src is unused); r.status: the entry's
// status word.  Everything is wave-uniform.
struct Step {
  Round r;
  uintptr_t base;  // the entry's input stream
  uint32_t span;   // bytes of the one range over it: consumed, or 0 where the round holds no full chunk
  uint32_t q0;     // the round's first payload chunk
  uint32_t k, j;   // the entry's slot; the output packet's index in its write (npk: none)
};

FUSED_DEV Geom geom_at(const CAS hdfs_relay_batch::Desc *p) {
  return Geom{p->g.stride, p->g.short_at, p->g.payload, p->g.cpp0,      p->g.hb0,
              p->g.K,      p->g.short_dlen, p->g.short_hb, p->g.empty};
}

FUSED_DEV Step step_at(const CAS hdfs_relay_batch::Desc *tab, const CAS uint32_t *pk0, uintptr_t status, uint32_t nw,
                       uint32_t total, uint32_t proto, uint32_t g, uint32_t &k, uint32_t wave) {
  const bool in = g < total;
  if (in) k = write_of(pk0, nw, g, k);
  const CAS hdfs_relay_batch::Desc *p = tab + k;
  const uint32_t npk = p->npk;
  Step s;
  s.k = k;
  s.j = in ? g - pk0[k] : npk;  // j == npk: no packet
  // the write's stream is a Write that starts on the chunk grid (n0 == 0): packet_at places its packets
  const Write w{nullptr, nullptr, p->wire, p->g.payload, p->off, p->seq, 0u, npk, p->hb, proto, 1u, p->finish, 0u};
  s.r.u = unit_of(w, s.j, wave);
  s.r.out0 = 0;
  s.r.sync = 0u;
  s.r.status = status + 4u * uintptr_t(k);
  s.base = reinterpret_cast<uintptr_t>(p->in.stream);
  s.span = s.r.u.nfr ? uint32_t(p->in.consumed) : 0u;  // consumed < 2^32
  s.q0 = s.j * kOutChunks + kRoundChunks * wave;
  return s;
}

// The round's registers from the input stream, and the wire bytes of its CRCs
// (lane 8c: chunk c's).  Piece k of the lane lies lo + 1024 k bytes into the
// round, so in chunk 2k + (lo >> 9) of it, (lo & 511) bytes in.  Chunks past the
// round's full ones, and lanes without a CRC to load, read offset 0 of the
// range: the registers are neither stored nor compared.
FUSED_DEV void load_seamed(u32x4 (&v)[4], uint32_t &wire, const CAS hdfs_relay_batch::Desc *p, const Step &s,
                           uint32_t lane, uint32_t lo) {
  const Geom g = geom_at(p);
  const __amdgpu_buffer_rsrc_t r = range_of(s.base, s.span);
  const uint32_t nfr = s.r.u.nfr;
  uint32_t so[kRoundChunks], co[kRoundChunks];
  Cursor c = seek(g, s.q0);
#pragma unroll
  for (uint32_t i = 0; i < kRoundChunks; i++) {
    so[i] = i < nfr ? uint32_t(data_at(g, c)) : 0u;
    co[i] = i < nfr ? uint32_t(crc_at(g, c)) : 0u;
    c = next_chunk(g, c);
  }
  const bool hi = (lo >> 9) != 0u;
  const uint32_t in = lo & (kGrid - 1u);
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) v[k] = load16(r, (hi ? so[2 * k + 1] : so[2 * k]) + in);
  const uint32_t sel = lane >> 3;
  uint32_t cw = 0u;
#pragma unroll
  for (uint32_t i = 0; i < kRoundChunks; i++) cw = ((lane & 7u) == 0u && sel == i) ? co[i] : cw;
  wire = load32(r, cw);
}

// The verified CRC words into the output packet's CRC region: lane 8c stores
// chunk c's (the range is exactly the round's CRC words).
FUSED_DEV void store_crcs(const Unit &u, uint32_t wave, uint32_t lane, uint32_t wire) {
  const __amdgpu_buffer_rsrc_t r = range_of(u.c0 + 4u * uintptr_t(kRoundChunks * wave), 4u * u.nfr);
  store32(r, (lane & 7u) == 0u ? 4u * (lane >> 3) : kNowhere, wire);
}

// Input packet i's header as the prediction composes it: what verify_header
// reads of a Round.
FUSED_DEV Round in_header(const CAS hdfs_relay_batch::Desc *p, uint32_t i) {
  const uint32_t nbody = p->in.nbody, dlen0 = p->in.dlen0;
  const bool body = i < nbody;
  const CAS PacketAt *t = p->in.tail + (body ? 0u : i - nbody);  // i - nbody < ntail <= kMaxTail
  Round r;
  Unit &u = r.u;
  u.p.off = body ? p->in.off0 + int64_t(uint64_t(i) * dlen0) : t->off;
  u.p.seq = body ? p->in.seq0 + int64_t(i) : t->seq;
  u.p.dlen = body ? dlen0 : t->dlen;
  u.p.ncrc = crc_count(u.p.dlen);
  u.p.last = body ? p->in.last0 : t->last;
  r.sync = body ? p->in.sync0 : t->sync;
  u.hb = body ? p->in.hb0 : t->hb;
  u.h0 = reinterpret_cast<uintptr_t>(p->in.stream) + (body ? uint64_t(i) * p->in.stride : t->stream_off);
  return r;
}

// The input headers output packet j of the entry answers for, dealt over the
// workgroup's waves: wave v takes the v-th, the (v + 16)-th, ...
FUSED_DEV bool check_headers(uint32_t *hdr, const CAS hdfs_relay_batch::Desc *p, uint32_t proto, uint32_t j,
                             uint32_t wave, uint32_t lane) {
  const Geom g = geom_at(p);
  const uint32_t all = p->in.npk, to = end_header(g, j, p->npk), end = to < all ? to : all;  // in_header's bound
  bool bad = false;
  for (uint32_t i = first_header(g, j) + wave; i < end; i += kWaves) bad |= verify_header(hdr, proto, in_header(p, i), lane);
  return bad;
}

// The output packet's chunk shorter than 512 B (n bytes behind its full chunks,
// n = 0: none), by one whole wave: the bytes from their place in the input
// (ragged_chunk's loads), stored behind the packet's full chunks,
// ragged_finish's lane arithmetic once, the CRC compared with the input's and
// stored into the output's CRC region.
FUSED_DEV bool relay_ragged(const uint32_t *img, const uint32_t *tab, const CAS hdfs_relay_batch::Desc *p,
                            const Step &s, uint32_t lane) {
  const Unit &u = s.r.u;
  const uint32_t nfull = u.p.dlen / kGrid, n = u.p.dlen % kGrid, pad = kGrid - n;
  const Geom g = geom_at(p);
  const Cursor c = seek(g, uint32_t(g.payload / kGrid));  // the payload's last, short chunk (n != 0: it has one)
  const __amdgpu_buffer_rsrc_t rs = range_of(s.base + uintptr_t(n ? data_at(g, c) : 0u), n);
  const uint32_t wire =
      load32(range_of(s.base + uintptr_t(n ? crc_at(g, c) : 0u), n ? 4u : 0u), lane == 0u ? 0u : kNowhere);
  uint32_t b[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) b[j] = load8(rs, 8u * lane + j - pad) & 0xFFu;
  const __amdgpu_buffer_rsrc_t rd = range_of(u.d0 + uintptr_t(kGrid) * nfull, n);
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) store8(rd, 8u * lane + j - pad, b[j]);
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
  store32(range_of(u.c0 + 4u * uintptr_t(nfull), n ? 4u : 0u), lane == 0u ? 0u : kNowhere, val);
  return lane == 0u && n != 0u && wire != val;
}

__global__ __launch_bounds__(1024) void relay_fused_batch_kernel(const CAS hdfs_relay_batch::Desc *dt,
                                                                 const CAS uint32_t *pk0, const CAS uint32_t *meta,
                                                                 uint32_t *status, uint32_t proto,
                                                                 const uint32_t *__restrict__ tab) {
  extern __shared__ uint32_t lds[];
  const uint32_t nw = meta[0], total = meta[1];
  if (blockIdx.x >= total) return;  // uniform: no packet for this workgroup (so nw >= 1 below)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  uint32_t *hdr = lds + crc::kImageWords + kExpectWords * wave;
  fill_image(lds, tab, tid);
  const uint32_t init512 = tab[crc::kCompactInit + kGrid];
  __syncthreads();
  const uint32_t lo = 64u * (lane & 15u) + 16u * (lane >> 4);
  const uint32_t G = gridDim.x;
  const uintptr_t st = reinterpret_cast<uintptr_t>(status);
  uint32_t g = blockIdx.x, k = 0u;
  // Two register sets take turns, as in frame_fused_batch_kernel.
  u32x4 ra[4], rb[4];
  uint32_t wa, wb;
  Step s = step_at(dt, pk0, st, nw, total, proto, g, k, wave);
  load_seamed(ra, wa, dt + s.k, s, lane, lo);
  auto step = [&](const u32x4(&cur)[4], uint32_t wcur, u32x4(&nxt)[4], uint32_t &wnxt) {
    const Step sn = step_at(dt, pk0, st, nw, total, proto, g + G, k, wave);  // g + G < 2^32: total < 2^29, G <= 1024
    load_seamed(nxt, wnxt, dt + sn.k, sn, lane, lo);  // the next packet's loads, ahead of this round's stores
    const Unit &u = s.r.u;
    store_round(cur, u, lo);
    bool bad = verify_round(lds, cur, wcur, u, lane, init512);
    store_crcs(u, wave, lane, wcur);
    bad |= check_headers(hdr, dt + s.k, proto, s.j, wave, lane);
    if (wave == 0u) {
      header(hdr, proto, u, lane);
      bad |= relay_ragged(lds, tab, dt + s.k, s, lane);
    }
    flag(s.r, bad);
    g += G;
    s = sn;
  };
  while (g < total) {
    step(ra, wa, rb, wb);
    if (g >= total) break;
    step(rb, wb, ra, wa);
  }
}

hipError_t prepare_relay_fused_batch() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&relay_fused_batch_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kExpectWords * kWaves) * sizeof(uint32_t)));
}

hipError_t launch_probe(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(probe_relay_kernel, dim3(1), dim3(kMaxEntries), 0, stream,
                     reinterpret_cast<const hdfs_relay_batch::Entry *>(b + t.in), n, proto, chunk_size, ctype,
                     reinterpret_cast<hdfs_relay_batch::Desc *>(b + t.desc), reinterpret_cast<uint32_t *>(b + t.slot),
                     reinterpret_cast<uint32_t *>(b + t.status), reinterpret_cast<uint32_t *>(b + t.pk0),
                     reinterpret_cast<uint32_t *>(b + t.meta));
  return hipGetLastError();
}

hipError_t launch_relay_fused_batch(void *tables, uint32_t n, uint32_t proto, const uint32_t *crc_tab, uint32_t groups,
                                    hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !groups || groups > kBatchMaxGroups || !crc_tab)
    return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(relay_fused_batch_kernel, dim3(groups), dim3(64 * kWaves),
                     (crc::kImageWords + kExpectWords * kWaves) * sizeof(uint32_t), stream,
                     (const CAS hdfs_relay_batch::Desc *)(b + t.desc), (const CAS uint32_t *)(b + t.pk0),
                     (const CAS uint32_t *)(b + t.meta), reinterpret_cast<uint32_t *>(b + t.status), proto, crc_tab);
  return hipGetLastError();
}

}  // namespace hdfs_relay_batch
