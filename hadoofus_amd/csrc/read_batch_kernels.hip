// A batch of block reads on gfx950 in two launches and ONE pass over the
// bytes: probe_kernel, then unframe_fused_batch_kernel.
//
// probe_kernel is one workgroup, thread e for entry e.  It frames packet 0 of
// its entry's stream with frame::frame_step, derives the stride and the packet
// count, frames the tail, and decides whether the entry is regular
// (read_batch_layout.h: all of that arithmetic is probe_entry's, which the CPU
// suite runs on host streams).  Then thread 0 lays the packet-count prefix
// over the regular entries (prefix_regular), and every regular entry's
// descriptor goes to its slot, its status word set to 0.  Irregular entries
// get no slot and no packets: the main launch never touches them.
//
// unframe_fused_batch_kernel is frame_fused_batch_kernel
// (wire_fused_batch_kernels.hip) run backwards, with the same round
// (wire_fused_round.h): a workgroup is 16 waves, the table image is filled
// once per workgroup behind the only barrier, workgroup b walks global packets
// g = b, b + G, ... of the regular entries, found with write_of
// (wire_fused_batch_lookup.h) on the prefix array through the constant address
// space.  Wave v takes round v (4 KiB, eight chunks) of the packet: four
// coalesced 16-B loads from the packet's data region in the stream
// (load_round), the same registers stored straight out to the destination
// (store_round), the in-register transpose and wire_fused_crc.h's lane
// arithmetic; lane 8c compares chunk c's CRC with the four wire bytes of the
// packet's CRC region.  Wave 0 also composes the header it expects
// (outpkt::put_out_header, plus the syncBlock bytes of a 33-byte header) and
// compares it with the stream's, a byte per lane, and verifies and copies the
// chunk shorter than 512 B in ragged_chunk's zero frame.  Two register sets
// take turns, and the next packet's loads are issued ahead of the current
// round's stores.
//
// Any mismatch makes the lane that saw it store 1 into its entry's status
// word: a plain vector store, every writer the same value.  No atomics, no
// spinning, no cross-workgroup dependence.  The host hands a flagged entry to
// hdfs_crc32c_read_packets, which overwrites its destination.
//
// SAFETY.  Every address of the main launch comes from the probe's descriptor:
// a packet's header, CRC and data regions lie at stream_off + [0, hb + 4 ncrc +
// dlen) and its destination at dst_off + [0, dlen).  The probe validated
// nbody * stride + tail == consumed <= len and delivered <= dst_cap, with
// every packet inside (read_batch_layout.h), from the lengths alone.  Every
// vector access goes through range_of over exactly the bytes it may touch --
// the round's full chunks, the packet's header, its CRC words, its ragged
// chunk, the entry's status word -- and the hardware drops what falls outside.
// So whatever the stream's bytes are, and they may change under the kernel, no
// load leaves [stream, stream + len) and no store leaves [dst, dst + dst_cap)
// or the status array: a corrupt stream costs a fallback, never an access out
// of range.  The probe's own loads are frame_step's: at most min(rem, 6 +
// hlen) bytes at a position below len.  The host checked that every range lies
// inside one device allocation and that no destination overlaps a stream or
// another destination, so no byte a wave loads is one another wave stores.
#include "crc32c_frame.h"
#include "crc32c_outpkt.h"
#include "read_batch_internal.h"
#include "read_batch_layout.h"
#include "read_batch_verify.h"
#include "wire_fused_batch_lookup.h"
#include "wire_fused_round.h"

namespace hdfs_read_batch {

#define CAS __attribute__((address_space(4)))

constexpr uint32_t kExpectWords = 16;  // the expected header, 33 bytes at most; every lane reads a byte of it

// ---- the probe ----------------------------------------------------------------------
struct DeviceBytes {
  const uint8_t *s;
  __host__ __device__ const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

__global__ __launch_bounds__(1024) void probe_kernel(const Entry *__restrict__ in, uint32_t n, int proto,
                                                     uint32_t chunk_size, int ctype, uint32_t want_records,
                                                     uint64_t max_pkts, Desc *__restrict__ desc,
                                                     uint32_t *__restrict__ slot, uint32_t *__restrict__ status,
                                                     uint32_t *__restrict__ pk0, uint32_t *__restrict__ meta) {
  __shared__ uint32_t npk[kMaxEntries], at[kMaxEntries];
  const uint32_t e = threadIdx.x;
  Desc d;
  bool regular = false;
  if (e < n) {
    const Entry x = in[e];
    regular = probe_entry(DeviceBytes{x.stream}, x.len, x.dst_cap, proto, chunk_size, ctype, want_records != 0u,
                          max_pkts, d);
    d.stream = x.stream;
    d.dst = x.dst;
    d.entry = e;
  }
  npk[e] = regular ? d.npk : 0u;
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
FUSED_DEV Round round_at(const CAS Desc *tab, const CAS uint32_t *pk0, uintptr_t status, uint32_t nw, uint32_t total,
                         uint32_t g, uint32_t &k, uint32_t wave) {
  const bool in = g < total;
  if (in) k = write_of(pk0, nw, g, k);
  const CAS Desc *p = tab + k;
  const uint32_t i = in ? g - pk0[k] : 0u, nbody = p->nbody;
  const bool body = i < nbody;
  const CAS PacketAt *t = p->tail + (body ? 0u : i - nbody);  // i - nbody < ntail <= kMaxTail
  const uint32_t dlen0 = p->dlen0;
  const uint64_t soff = body ? uint64_t(i) * p->stride : t->stream_off;
  const uint64_t doff = body ? uint64_t(i) * dlen0 : t->dst_off;
  Round r;
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
  r.out0 = reinterpret_cast<uintptr_t>(p->dst) + doff;
  u.dst = r.out0 + uintptr_t(kRound) * wave;
  r.status = status + 4u * uintptr_t(k);
  return r;
}

// The packet's header, by one whole wave: lane 0 composes the expected one
// into LDS, lane t compares byte t with the stream's.
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
// 0: none), by one whole wave: ragged_chunk's loads from the stream's data
// region, ragged_finish's lane arithmetic, the bytes stored to the destination
// and the CRC compared with the stream's.
FUSED_DEV bool verify_ragged(const uint32_t *img, const uint32_t *tab, const Round &r, uint32_t lane) {
  const Unit &u = r.u;
  const uint32_t nfull = u.p.dlen / kChunk, n = u.p.dlen % kChunk, pad = kChunk - n;
  const __amdgpu_buffer_rsrc_t rs = range_of(u.d0 + uintptr_t(kChunk) * nfull, n);
  const uint32_t wire = load32(range_of(u.c0 + 4u * uintptr_t(nfull), n ? 4u : 0u), lane == 0u ? 0u : kNowhere);
  uint32_t b[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) b[j] = load8(rs, 8u * lane + j - pad) & 0xFFu;
  const __amdgpu_buffer_rsrc_t rd = range_of(r.out0 + uintptr_t(kChunk) * nfull, n);
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
  return lane == 0u && n != 0u && wire != val;
}

__global__ __launch_bounds__(1024) void unframe_fused_batch_kernel(const CAS Desc *dt, const CAS uint32_t *pk0,
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
  // Two register sets take turns, as in frame_fused_batch_kernel.
  u32x4 ra[4], rb[4];
  uint32_t wa, wb;
  Round r = round_at(dt, pk0, st, nw, total, g, k, wave);
  load_round(ra, r.u, lo);
  wa = load_crcs(r.u, wave, lane);
  auto step = [&](const u32x4(&cur)[4], uint32_t wcur, u32x4(&nxt)[4], uint32_t &wnxt) {
    const Round rn = round_at(dt, pk0, st, nw, total, g + G, k, wave);  // g + G < 2^32: total < 2^29, G <= 1024
    load_round(nxt, rn.u, lo);  // the next packet's loads, ahead of this round's stores
    wnxt = load_crcs(rn.u, wave, lane);
    store_round(cur, r.u, lo);
    bool bad = verify_round(lds, cur, wcur, r.u, lane, init512);
    if (wave == 0u) {
      bad |= verify_header(hdr, proto, r, lane);
      bad |= verify_ragged(lds, tab, r, lane);
    }
    flag(r, bad);
    g += G;
    r = rn;
  };
  while (g < total) {
    step(ra, wa, rb, wb);
    if (g >= total) break;
    step(rb, wb, ra, wa);
  }
}

hipError_t prepare_unframe_fused_batch() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&unframe_fused_batch_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kExpectWords) * sizeof(uint32_t)));
}

hipError_t launch_probe(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype, bool want_records,
                        uint64_t max_pkts, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(kMaxEntries), 0, stream, reinterpret_cast<const Entry *>(b + t.in), n,
                     proto, chunk_size, ctype, want_records ? 1u : 0u, max_pkts, reinterpret_cast<Desc *>(b + t.desc),
                     reinterpret_cast<uint32_t *>(b + t.slot), reinterpret_cast<uint32_t *>(b + t.status),
                     reinterpret_cast<uint32_t *>(b + t.pk0), reinterpret_cast<uint32_t *>(b + t.meta));
  return hipGetLastError();
}

hipError_t launch_unframe_fused_batch(void *tables, uint32_t n, uint32_t proto, const uint32_t *crc_tab,
                                      uint32_t groups, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !groups || groups > kBatchMaxGroups || !crc_tab)
    return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(unframe_fused_batch_kernel, dim3(groups), dim3(64 * kWaves),
                     (crc::kImageWords + kExpectWords) * sizeof(uint32_t), stream, (const CAS Desc *)(b + t.desc),
                     (const CAS uint32_t *)(b + t.pk0), (const CAS uint32_t *)(b + t.meta),
                     reinterpret_cast<uint32_t *>(b + t.status), proto, crc_tab);
  return hipGetLastError();
}

}  // namespace hdfs_read_batch
