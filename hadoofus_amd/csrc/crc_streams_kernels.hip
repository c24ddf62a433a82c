// Composite CRCs from packet streams on gfx950 in three launches on one stream:
// probe_streams_kernel, fold_packets_kernel, reduce_entries_kernel (DESIGN.md
// section 24).  No byte of a packet's data is read.
//
// probe_streams_kernel is the read batch library's probe: one workgroup, thread
// e for entry e, read_batch_layout.h's probe_entry as it stands (no destination,
// so dst_cap is without limit, and no records), prefix_regular for the slots and
// the packet-count prefix.  There is no framing arithmetic here.
//
// fold_packets_kernel takes a packet a wave and step, packets g = w, w + W, ...
// of the regular entries, found with the lookup of wire_fused_batch_lookup.h on
// the packet-count prefix through the constant address space.  The wave first
// compares the packet's header with the one the prediction composes
// (read_batch_header.h's verify_header); a mismatch makes the lane that saw it
// store 1 into its entry's status word: a plain vector store, every writer the
// same value.  Then it folds the packet's CRC region, which lies directly
// behind that header, into the packet's own CRC (crc_streams_lookup.h: THE
// FOLD): the lanes load the CRC words through one buffer range over exactly the
// region's bytes -- the wave owns one packet, so one descriptor in scalar
// registers serves any byte address, and a lane without a chunk loads zero from
// outside the range -- multiply, and XOR-reduce; lane 0 stores the packet's
// CRC into the library's per-packet table at the global packet number.  One
// writer a word, so no atomics, no spinning, no cross-workgroup dependence.
//
// reduce_entries_kernel takes an entry a wave: the lanes run Horner's scheme
// over contiguous runs of the entry's packets (lookup.h: THE REDUCE), are
// advanced past the bytes behind their runs, XOR-reduced, and lane 0 stores the
// entry's CRC at its slot.  A flagged slot is skipped: the host takes the
// fallback.
//
// THE DESCRIBED-PACKET PATH.  Entries that are irregular or flagged are framed
// on the host by hdfs_crc32c_parse_packets; its records become a table of
// (CRC region, CRC count, data length, payload behind).  The same two kernels
// take that table instead of the probe's descriptors (recs != NULL): the same
// fold, the same reduce, no header check (the walk framed every header).
//
// MULTIPLIES, NOT BYTE TABLES.  Every product is a branch-free GF(2) multiply
// (lookup.h: mulmod, about 160 VALU operations); the multipliers are 129 words
// made on the host with crc32c_tables.h's operator.  The fold costs one
// multiply a chunk behind a packet's first 64 and three a packet, the fold
// kernel holds no LDS but the expected headers, and a table of LDS byte lookups
// (four a multiply, 4 KiB a multiplier) would have to be filled by every
// workgroup for 66 multipliers.  That count does not settle the step word, the
// one multiplier inside the per-chunk loop, which a 4 KiB table would serve:
// no A/B of the two was run, and it stays open work (not
// measured).
//
// SAFETY.  Every trip count and address follows from the probe's descriptor,
// that is from lengths validated against len (nbody * stride + tail ==
// consumed <= len, every packet inside), or from hdfs_crc32c_parse_packets'
// records, never from stream bytes: no load leaves [stream, stream +
// consumed), of it no data byte is loaded, and a corrupt stream costs a
// fallback, never an access out of range or an unbounded loop.  Every load of
// stream bytes goes through range_of over exactly the header's or the CRC
// region's bytes.  The per-packet table is written below `cap` only.  Nothing
// is stored but the library's own tables.  No kernel has a private segment or
// a vector register spill, and the fold and the reduce spill no scalar register.
// THE PROBE SPILLS 59 SCALAR REGISTERS into lanes of vector registers
// (v_writelane; none to memory): it is probe_entry as it stands, inlined three
// frame_steps deep, one workgroup run once a call, and is accepted as it is in
// the libraries that share it; tests/test_crc_streams_cpu.py pins the count.
#include "crc32c_frame.h"
#include "crc32c_outpkt.h"
#include "crc_streams_internal.h"
#include "crc_streams_lookup.h"
#include "read_batch_header.h"
#include "read_batch_layout.h"
#include "read_batch_verify.h"
#include "wire_fused_batch_lookup.h"

namespace hdfs_crc_streams {

#define CAS __attribute__((address_space(4)))

using hdfs_read_batch::PacketAt;
using hdfs_read_batch::Round;
using hdfs_wire_fused::kNowhere;
using hdfs_wire_fused::range_of;
using hdfs_wire_fused::rfl;
using hdfs_wire_fused::write_of;

// ---- the probe ----------------------------------------------------------------------
struct DeviceBytes {
  const uint8_t *s;
  __host__ __device__ const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

__global__ __launch_bounds__(1024) void probe_streams_kernel(const Entry *__restrict__ in, uint32_t n, int proto,
                                                             uint32_t chunk_size, int ctype, Desc *__restrict__ desc,
                                                             uint32_t *__restrict__ slot,
                                                             uint32_t *__restrict__ status,
                                                             uint32_t *__restrict__ pk0,
                                                             uint32_t *__restrict__ meta) {
  __shared__ uint32_t npk[kMaxEntries], at[kMaxEntries];
  const uint32_t e = threadIdx.x;
  Desc d;
  bool regular = false;
  if (e < n) {
    const Entry x = in[e];
    regular = hdfs_read_batch::probe_entry(DeviceBytes{x.stream}, x.len, ~uint64_t(0), proto, chunk_size, ctype, false,
                                           0, d);
    d.stream = x.stream;
    d.dst = nullptr;
    d.entry = e;
  }
  npk[e] = regular ? d.npk : 0u;
  __syncthreads();
  if (e == 0u) {
    const uint32_t nreg = hdfs_read_batch::prefix_regular(npk, n, at, pk0);
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

// ---- check and fold -----------------------------------------------------------------
// Packet g of the regular entries as the comparison takes it (wave-uniform).
FUSED_DEV Round packet_round(const CAS Desc *tab, const CAS uint32_t *pk0, uintptr_t status, uint32_t nw, uint32_t g,
                             uint32_t &k) {
  k = write_of(pk0, nw, g, k);
  const CAS Desc *p = tab + k;
  const uint32_t i = g - pk0[k], nbody = p->nbody;
  const bool body = i < nbody;
  const CAS PacketAt *t = p->tail + (body ? 0u : (i - nbody < kTailPackets ? i - nbody : 0u));
  const uint32_t dlen0 = p->dlen0;
  Round r;
  hdfs_wire_fused::Unit &u = r.u;
  u.p.wire_off = body ? uint64_t(i) * p->stride : t->stream_off;
  u.p.data_off = 0u;
  u.p.off = body ? p->off0 + int64_t(uint64_t(i) * dlen0) : t->off;
  u.p.seq = body ? p->seq0 + int64_t(i) : t->seq;
  u.p.dlen = body ? dlen0 : t->dlen;
  u.p.ncrc = hdfs_read_batch::crc_count(u.p.dlen);
  u.p.cidx = 0u;
  u.p.last = body ? p->last0 : t->last;
  r.sync = body ? p->sync0 : t->sync;
  u.hb = body ? p->hb0 : t->hb;
  u.h0 = reinterpret_cast<uintptr_t>(p->stream) + u.p.wire_off;
  u.c0 = u.h0 + u.hb;
  u.d0 = u.src = u.dst = 0u;
  u.nfr = 0u;
  r.out0 = 0u;
  r.status = status + 4u * uintptr_t(k);
  return r;
}

// XOR of the wave's 64 lanes, in every lane.
FUSED_DEV uint32_t xor_lanes(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v ^= __shfl_xor(v, off);
  return v;
}

// The CRC of the packet whose ncrc CRC words lie at c0 (any byte address), by
// one whole wave; the same value in every lane.
FUSED_DEV uint32_t fold_region(uintptr_t c0, uint32_t ncrc, uint32_t dlen, const CAS uint32_t *mult, uint32_t mlane,
                               uint32_t lane) {
  const uint32_t poly = mult[kMultPoly], mstep = mult[kMultStep];
  const Chunks ch = chunks_of(ncrc, dlen, mult[kMultChunk]);
  const __amdgpu_buffer_rsrc_t rg = range_of(c0, 4u * ncrc);  // 4 ncrc is a record's crc_len: below 2^31
  uint32_t a = 0u;
  for (uint32_t s = 0; s < ch.steps; s++) {
    const uint32_t i = chunk_at(ch, s, lane);
    a = fold_step(a, hdfs_read_batch::load32(rg, i != kNoChunk ? 4u * i : kNowhere), s, mstep, poly);
  }
  const uint32_t front = xor_lanes(mulmod(a, mlane, poly));
  const uint32_t last = hdfs_read_batch::load32(rg, ncrc ? 4u * (ncrc - 1u) : kNowhere);
  return packet_crc(ch, front, last, xpow8(mult + kMultPow2, ch.last_len, poly), poly);
}

__global__ __launch_bounds__(64 * kFoldWaves) void fold_packets_kernel(const CAS Desc *dt, const CAS uint32_t *pk0,
                                                                       const CAS uint32_t *meta, uint32_t *status,
                                                                       const CAS PktRec *recs, uint32_t nrec,
                                                                       const CAS uint32_t *mult, uint32_t proto,
                                                                       uint32_t cap, uint32_t *__restrict__ cp) {
  __shared__ uint32_t expect[kFoldWaves][16];  // the expected header, 33 bytes at most, one per wave
  const bool described = recs != nullptr;
  const uint32_t nw = described ? 0u : meta[0], total = described ? nrec : meta[1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  const uint32_t W = gridDim.x * kFoldWaves;  // <= 2^13; total < 2^29, so g + W does not wrap
  const uintptr_t st = reinterpret_cast<uintptr_t>(status);
  const uint32_t mlane = mult[kMultLane + lane];
  uint32_t k = 0u;
  for (uint32_t g = blockIdx.x * kFoldWaves + wave; g < total; g += W) {
    uintptr_t c0;
    uint32_t ncrc, dlen;
    if (described) {
      const CAS PktRec *p = recs + g;
      c0 = uintptr_t(p->addr);
      ncrc = p->ncrc;
      dlen = p->dlen;
    } else {
      const Round r = packet_round(dt, pk0, st, nw, g, k);
      const bool bad = hdfs_read_batch::verify_header(expect[wave], proto, r, lane);
      hdfs_read_batch::flag(r, bad || g >= cap);  // no room in the table: the entry takes the fallback
      c0 = r.u.c0;
      ncrc = r.u.p.ncrc;
      dlen = r.u.p.dlen;
    }
    if (g >= cap) continue;  // uniform
    const uint32_t c = fold_region(c0, ncrc, dlen, mult, mlane, lane);
    if (lane == 0u) cp[g] = c;
  }
}

// ---- the reduce ------------------------------------------------------------------------
__global__ __launch_bounds__(64) void reduce_entries_kernel(const Desc *__restrict__ desc,
                                                            const uint32_t *__restrict__ pk0,
                                                            const uint32_t *__restrict__ status,
                                                            const uint32_t *__restrict__ meta,
                                                            const Span *__restrict__ spans,
                                                            const PktRec *__restrict__ recs, uint32_t count,
                                                            const CAS uint32_t *mult,
                                                            const uint32_t *__restrict__ cp, uint32_t cap,
                                                            uint32_t *__restrict__ out) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  const bool described = spans != nullptr;
  if (s >= count || (!described && s >= meta[0])) return;
  const uint32_t poly = mult[kMultPoly];
  const CAS uint32_t *pow2 = mult + kMultPow2;
  uint32_t p0, npk;
  Shape sh = Shape{};
  if (described) {
    p0 = spans[s].p0;
    npk = spans[s].npk;
  } else {
    if (status[s]) return;  // flagged by the fold: the host takes the fallback
    p0 = pk0[s];
    npk = desc[s].npk;
    sh = shape_of(desc[s]);
    if (npk != sh.nbody + sh.ntail) return;
  }
  if (p0 > cap || npk > cap - p0) return;  // its packets are not all in the table
  // the body's multiplier is one constant per entry, the tail's three come from the descriptor
  const uint32_t x0 = xpow8(pow2, sh.dlen0, poly), xt0 = xpow8(pow2, sh.tail0, poly),
                 xt1 = xpow8(pow2, sh.tail1, poly), xt2 = xpow8(pow2, sh.tail2, poly);
  const uint32_t first = run_first(npk, lane), end = first + run_count(npk, lane);
  uint32_t acc = 0u;
  for (uint32_t i = first; i < end; i++) {
    uint32_t m;
    if (described) {
      m = xpow8(pow2, recs[p0 + i].dlen, poly);
    } else {
      const uint32_t t = i - sh.nbody;
      m = i < sh.nbody ? x0 : t == 0u ? xt0 : t == 1u ? xt1 : xt2;
    }
    acc = mulmod(acc, m, poly) ^ cp[p0 + i];
  }
  uint64_t behind = 0u;
  if (end > first) behind = described ? recs[p0 + end - 1u].after : bytes_before(sh, npk) - bytes_before(sh, end);
  acc = xor_lanes(advance(pow2, acc, behind, poly));
  if (lane == 0u) out[s] = acc;
}

// ---- launches -------------------------------------------------------------------------
hipError_t launch_probe_streams(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype,
                                hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(probe_streams_kernel, dim3(1), dim3(kMaxEntries), 0, stream,
                     reinterpret_cast<const Entry *>(b + t.in), n, proto, chunk_size, ctype,
                     reinterpret_cast<Desc *>(b + t.desc), reinterpret_cast<uint32_t *>(b + t.slot),
                     reinterpret_cast<uint32_t *>(b + t.status), reinterpret_cast<uint32_t *>(b + t.pk0),
                     reinterpret_cast<uint32_t *>(b + t.meta));
  return hipGetLastError();
}

hipError_t launch_fold_streams(void *tables, uint32_t n, uint32_t proto, uint32_t groups, uint32_t *cp, uint32_t cap,
                               hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !groups || groups > kFoldMaxGroups || !cp || !cap)
    return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(fold_packets_kernel, dim3(groups), dim3(64 * kFoldWaves), 0, stream,
                     (const CAS Desc *)(b + t.desc), (const CAS uint32_t *)(b + t.pk0),
                     (const CAS uint32_t *)(b + t.meta), reinterpret_cast<uint32_t *>(b + t.status),
                     (const CAS PktRec *)nullptr, 0u, (const CAS uint32_t *)(b + t.mult), proto, cap, cp);
  return hipGetLastError();
}

hipError_t launch_reduce_streams(void *tables, uint32_t n, const uint32_t *cp, uint32_t cap, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !cp) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(reduce_entries_kernel, dim3(n), dim3(64), 0, stream, reinterpret_cast<const Desc *>(b + t.desc),
                     reinterpret_cast<const uint32_t *>(b + t.pk0), reinterpret_cast<const uint32_t *>(b + t.status),
                     reinterpret_cast<const uint32_t *>(b + t.meta), static_cast<const Span *>(nullptr),
                     static_cast<const PktRec *>(nullptr), n, (const CAS uint32_t *)(b + t.mult), cp, cap,
                     reinterpret_cast<uint32_t *>(b + t.crc));
  return hipGetLastError();
}

hipError_t launch_fold_described(const PktRec *recs, uint32_t nrec, const uint32_t *mult, uint32_t groups, uint32_t *cp,
                                 hipStream_t stream) {
  if (!recs || !nrec || !mult || !groups || groups > kFoldMaxGroups || !cp) return hipErrorInvalidValue;
  hipLaunchKernelGGL(fold_packets_kernel, dim3(groups), dim3(64 * kFoldWaves), 0, stream, (const CAS Desc *)nullptr,
                     (const CAS uint32_t *)nullptr, (const CAS uint32_t *)nullptr, static_cast<uint32_t *>(nullptr),
                     (const CAS PktRec *)recs, nrec, (const CAS uint32_t *)mult, 0u, nrec, cp);
  return hipGetLastError();
}

hipError_t launch_reduce_described(const Span *spans, uint32_t nspan, const PktRec *recs, uint32_t nrec,
                                   const uint32_t *mult, const uint32_t *cp, uint32_t *out, hipStream_t stream) {
  if (!spans || !nspan || !recs || !mult || !cp || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(reduce_entries_kernel, dim3(nspan), dim3(64), 0, stream, static_cast<const Desc *>(nullptr),
                     static_cast<const uint32_t *>(nullptr), static_cast<const uint32_t *>(nullptr),
                     static_cast<const uint32_t *>(nullptr), spans, recs, nspan, (const CAS uint32_t *)mult, cp, nrec,
                     out);
  return hipGetLastError();
}

}  // namespace hdfs_crc_streams
