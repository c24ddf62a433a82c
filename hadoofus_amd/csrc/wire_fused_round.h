// One round of the fused framing kernels on gfx950: what frame_fused_kernel
// (wire_fused_kernels.hip, one write per launch) and frame_fused_batch_kernel
// (wire_fused_batch_kernels.hip, a batch of writes per launch) both run for a
// packet, so there is one definition of it.  Device code; hipcc only.  The
// two kernels differ only in how a workgroup finds its next packet and the
// write it belongs to; everything below takes the packet as a Unit and never
// sees a Write again: unit_of is the only place one is live.
// frame_fused_gather_kernel (wirev_fused_kernels.hip, a write held in
// fragments) runs the same round with a source of its own: it changes a
// Unit's src, loads a round with a fragment boundary inside by its own code
// into the registers load_round would have filled, and ends its ragged chunk
// in ragged_finish.
//
// A wave's round of a packet is 4 KiB of the packet's full chunks: four
// coalesced 16-B loads (load_round), the same registers stored straight out
// (store_round), the in-register transpose and wire_fused_crc.h's lane
// arithmetic (crc_round).  Wave 0 of the packet's workgroup also composes and
// stores the header (header) and copies the packet's chunk shorter than 512 B
// with its CRC (ragged_chunk).  Every vector-memory access goes through a
// buffer descriptor over exactly the bytes it may touch (range_of).
#ifndef HADOOFUS_WIRE_FUSED_ROUND_H
#define HADOOFUS_WIRE_FUSED_ROUND_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32c_outpkt.h"
#include "wire_fused_crc.h"
#include "wire_internal.h"

namespace hdfs_wire_fused {

using hdfs_wire::kChunk;
using hdfs_wire::packet_at;
using hdfs_wire::Pkt;
using hdfs_wire::Write;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
#define FUSED_DEV static __device__ __forceinline__

constexpr uint32_t kWaves = 16, kRound = 4096, kRoundChunks = 8;
constexpr uint32_t kHdrWords = 8;  // 31 header bytes
constexpr uint32_t kNowhere = 0x80000000u;  // an offset outside every range: the access is dropped

FUSED_DEV uint32_t rfl(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

// Every vector-memory access of the kernel goes through a buffer descriptor
// over exactly the bytes it may touch: [a, a + bytes), at any byte address.
// An access outside the range is dropped by the hardware (a load gives
// zeros), so rounds past a packet's chunks need no branch: every wave issues
// the same vector-memory instructions in every iteration, in uniform control
// flow, and the compiler's s_waitcnt vmcnt(N) stay counted.
FUSED_DEV __amdgpu_buffer_rsrc_t range_of(uintptr_t a, uint32_t bytes) {
  const uint64_t u = (uint64_t(rfl(uint32_t(uint64_t(a) >> 32))) << 32) | rfl(uint32_t(a));
  return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(u), 0, int(rfl(bytes)), 0x00020000);
}
// The cache policy of the 16-B accesses (aux: 2 = nt, 16 = sc1), as measured
// (DESIGN.md section 16); other values only in A/B builds.
#ifndef HDFS_FUSED_LOAD_AUX
#define HDFS_FUSED_LOAD_AUX 0
#endif
#ifndef HDFS_FUSED_STORE_AUX
#define HDFS_FUSED_STORE_AUX 2
#endif
FUSED_DEV u32x4 load16(__amdgpu_buffer_rsrc_t r, uint32_t o) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, o, 0, HDFS_FUSED_LOAD_AUX));
}
FUSED_DEV void store16(__amdgpu_buffer_rsrc_t r, uint32_t o, u32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(v, r, o, 0, HDFS_FUSED_STORE_AUX);
}
FUSED_DEV void store32(__amdgpu_buffer_rsrc_t r, uint32_t o, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b32(v, r, o, 0, 0);
}
FUSED_DEV uint32_t load8(__amdgpu_buffer_rsrc_t r, uint32_t o) {
  return __builtin_amdgcn_raw_buffer_load_b8(r, o, 0, 0);
}
FUSED_DEV void store8(__amdgpu_buffer_rsrc_t r, uint32_t o, uint32_t v) {
  __builtin_amdgcn_raw_buffer_store_b8(uint8_t(v), r, o, 0, 0);
}

template <int CTRL>
FUSED_DEV uint32_t dpp(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), CTRL, 0xF, 0xF, true));
}

// XOR of each group of eight lanes, in every lane of the group: quad_perm
// [1,0,3,2] and [2,3,0,1], then row_half_mirror (crc::chunk_fold across lanes).
FUSED_DEV uint32_t fold8(uint32_t v) {
  v ^= dpp<0xB1>(v);
  v ^= dpp<0x4E>(v);
  v ^= dpp<0x141>(v);
  return v;
}

// Register bit 0 <-> lane bit 4, then register bit 1 <-> lane bit 5: lane L,
// which loaded pieces 64k + 4 (L & 15) + (L >> 4), k = 0..3, holds pieces
// 4L .. 4L + 3 afterwards, dword 4k' + c of its 64 bytes in d[4k' + c].
FUSED_DEV void transpose(uint32_t (&d)[16]) {
#pragma unroll
  for (int c = 0; c < 4; c++) {
#pragma unroll
    for (int k = 0; k < 4; k += 2) {
      const auto r = __builtin_amdgcn_permlane16_swap(d[k * 4 + c], d[(k + 1) * 4 + c], false, false);
      d[k * 4 + c] = r[0];
      d[(k + 1) * 4 + c] = r[1];
    }
  }
#pragma unroll
  for (int c = 0; c < 4; c++) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const auto r = __builtin_amdgcn_permlane32_swap(d[k * 4 + c], d[(k + 2) * 4 + c], false, false);
      d[k * 4 + c] = r[0];
      d[(k + 2) * 4 + c] = r[1];
    }
  }
}

// The wave's round of packet i of a write: everything here is wave-uniform.
// i >= npk (no packet: past the workgroup's last one) is a round of nothing,
// every range empty.
struct Unit {
  Pkt p;
  uintptr_t h0, c0, d0;  // the packet's header, CRC and data regions in the stream
  uintptr_t src, dst;    // the round's first byte in the write and in the stream
  uint32_t nfr;          // full chunks of the packet in this round (0..8)
  uint32_t hb;           // header bytes to store (0: no packet)
};

FUSED_DEV Unit unit_of(const Write &w, uint32_t i, uint32_t wave) {
  Unit u;
  const bool is = i < w.npk;
  u.p = packet_at(w, is ? i : 0u);
  if (!is) u.p.dlen = u.p.ncrc = 0u;
  u.hb = is ? w.hb : 0u;
  u.h0 = reinterpret_cast<uintptr_t>(w.wire) + u.p.wire_off;
  u.c0 = u.h0 + w.hb;
  u.d0 = u.c0 + 4u * uintptr_t(u.p.ncrc);
  const uint32_t nfull = u.p.dlen / kChunk, first = kRoundChunks * wave;
  u.nfr = nfull > first ? (nfull - first < kRoundChunks ? nfull - first : kRoundChunks) : 0u;
  u.src = reinterpret_cast<uintptr_t>(w.data) + u.p.data_off + uintptr_t(kRound) * wave;
  u.dst = u.d0 + uintptr_t(kRound) * wave;
  return u;
}

// Piece k of the lane lies lo + 1024 k bytes into the round; the range is the
// round's full chunks, so a piece is wholly inside it or wholly outside.
FUSED_DEV void load_round(u32x4 (&v)[4], const Unit &u, uint32_t lo) {
  const __amdgpu_buffer_rsrc_t r = range_of(u.src, u.nfr * kChunk);
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) v[k] = load16(r, lo + 1024u * k);
}

FUSED_DEV void store_round(const u32x4 (&v)[4], const Unit &u, uint32_t lo) {
  const __amdgpu_buffer_rsrc_t r = range_of(u.dst, u.nfr * kChunk);
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) store16(r, lo + 1024u * k, v[k]);
}

// The CRCs of the round's full chunks, from the registers of its loads: lane
// 8c stores chunk c's.  The store is issued whatever nfr is (an empty range
// drops it).
template <bool CSUM>
FUSED_DEV void crc_round(const uint32_t *img, const u32x4 (&v)[4], const Unit &u, uint32_t wave, uint32_t lane,
                         uint32_t init512) {
  if (!CSUM) return;
  uint32_t val = 0u;
  if (u.nfr) {  // uniform; no vector-memory access inside
    uint32_t d[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      d[4 * k + 0] = v[k].x;
      d[4 * k + 1] = v[k].y;
      d[4 * k + 2] = v[k].z;
      d[4 * k + 3] = v[k].w;
    }
    transpose(d);
    val = crc::chunk_final(fold8(crc::piece_shift(img, lane & 7u, crc::piece_raw(img, lane, d))), init512);
  }
  const __amdgpu_buffer_rsrc_t r = range_of(u.c0 + 4u * uintptr_t(kRoundChunks * wave), 4u * u.nfr);
  store32(r, (lane & 7u) == 0u ? 4u * (lane >> 3) : kNowhere, val);
}

// The packet's header, by one whole wave: lane 0 composes it into LDS, lane t
// stores byte t.  proto holds for every packet of a launch.
FUSED_DEV void header(uint32_t *hdr, uint32_t proto, const Unit &u, uint32_t lane) {
  if (lane == 0u)
    hdfs_crc32c::outpkt::put_out_header(reinterpret_cast<uint8_t *>(hdr), int(proto), u.p.off, u.p.seq,
                                        u.p.last != 0u, int32_t(u.p.dlen), u.p.ncrc);
  // a wave's LDS operations execute in order; the fences keep the compiler from reordering them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t b = reinterpret_cast<const uint8_t *>(hdr)[lane & 31u];
  store8(range_of(u.h0, u.hb), lane, b);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The second half of ragged_chunk, for a kernel that loads the chunk's bytes
// its own way: b[j] is byte 8 lane + j of the zero frame (zero below pad).
// The bytes are stored behind the packet's full chunks, and the chunk's CRC.
template <bool CSUM>
FUSED_DEV void ragged_finish(const uint32_t *img, const uint32_t *tab, const uint32_t (&b)[8], const Unit &u,
                             uint32_t lane) {
  const uint32_t nfull = u.p.dlen / kChunk, n = u.p.dlen % kChunk, pad = kChunk - n;
  const __amdgpu_buffer_rsrc_t rd = range_of(u.d0 + uintptr_t(kChunk) * nfull, n);
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) store8(rd, 8u * lane + j - pad, b[j]);
  if (!CSUM) return;
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
}

// The packet's chunk shorter than 512 B (n bytes behind its full chunks, n =
// 0: none), by one whole wave: copied, and its CRC stored.  src0: the packet's
// first data byte in the write (wave 0's u.src; a kernel that has the write at
// hand may say it in the form that costs it fewest registers).  Byte f of the
// zero frame holds byte f - pad of the chunk; below pad the offset wraps out
// of the range.
template <bool CSUM>
FUSED_DEV void ragged_chunk(const uint32_t *img, const uint32_t *tab, uintptr_t src0, const Unit &u, uint32_t lane) {
  const uint32_t nfull = u.p.dlen / kChunk, n = u.p.dlen % kChunk, pad = kChunk - n;
  const __amdgpu_buffer_rsrc_t rs = range_of(src0 + uintptr_t(kChunk) * nfull, n);
  uint32_t b[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) b[j] = load8(rs, 8u * lane + j - pad);
  ragged_finish<CSUM>(img, tab, b, u, lane);
}

// The workgroup's table image (wire_fused_crc.h) from the compact tables at
// tab, by all 1024 threads: thread t replicates slicing entry t 32 times
// (eight 16-B writes), then the Z tables as they are.  The caller's barrier
// follows.
FUSED_DEV void fill_image(uint32_t *lds, const uint32_t *tab, uint32_t tid) {
  const uint32_t v = tab[crc::kCompactSlice + tid];
  u32x4 *p = reinterpret_cast<u32x4 *>(lds + crc::slice_at(tid >> 8, tid & 255u, 0u));
#pragma unroll
  for (int j = 0; j < 8; j++) p[j] = u32x4{v, v, v, v};
#pragma unroll
  for (uint32_t j = 0; j < 7; j++) lds[crc::kImageZ + 1024u * j + tid] = tab[crc::kCompactZ + 1024u * j + tid];
}

}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_ROUND_H
