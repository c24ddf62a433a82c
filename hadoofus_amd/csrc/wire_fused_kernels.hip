// A write's packets as one wire stream on gfx950 in ONE pass over the data:
// frame_fused_kernel copies a packet's data into the stream and computes the
// chunk CRCs from the registers it copies, so there is no CRC array, no compute
// plan and no second kernel.
//
// Work.  A workgroup is 16 waves; a full packet's data is 16 rounds of 4 KiB
// (eight 512-B chunks), so wave v of the workgroup takes round v of the
// packet.  Workgroup b takes packets b, b + G, b + 2G, ... of the write (G
// workgroups, about one per CU): a bound that is uniform per workgroup, no
// atomics, no waiting on another workgroup.  The workgroup fills its table
// image (wire_fused_crc.h: slicing-by-4 replicated 32x, 128 KiB, and the seven
// Z tables) once and then walks its packets.
//
// A round.  Four fully coalesced 1 KiB loads, lane L of load k holding 16-B
// piece 64k + 4 (L & 15) + (L >> 4) of the round -- the load order of the main
// library's tiled kernel -- at any byte address.  The registers go straight
// out to the packet's data region at the offsets they were loaded from, four
// coalesced 16-B stores (non-temporal) at any byte address.  Then the
// in-register transpose (v_permlane16_swap / v_permlane32_swap) leaves lane L
// with the 64 contiguous bytes of piece L & 7 of chunk L >> 3, and
// wire_fused_crc.h's lane arithmetic runs: 16 slicing steps, the shift
// Z_{64 (7 - i)}, the XOR of the chunk's eight lanes (DPP), the final
// inversion.  Lane 8c stores chunk c's four wire bytes into the packet's CRC
// region itself, at any byte address.  The loads of the wave's next packet are
// issued before the current round is stored, so they are in flight across the
// whole round.
//
// Ragged ends.  A round covers only the packet's FULL chunks: a piece of a
// chunk past them is neither loaded nor stored (a buffer descriptor's range,
// see range_of).  The at most two chunks of a write shorter than 512 B (the
// short first packet, the write's last chunk) are wave 0's of the packet's
// workgroup: lane L loads and stores bytes [8L, 8L + 8) of the chunk
// right-aligned in a zero frame of 512 B, and eight lanes gather the frame's
// pieces with ds_bpermute and run the same lane arithmetic.  Wave 0 also
// composes the packet's header (outpkt::put_out_header, one lane, into LDS)
// and stores it, a byte a lane.
//
// Invariants.  Every byte of [wire, wire + wire_len) is stored exactly once:
// the packets tile the stream (wire_layout.h checks that on the host); of a
// packet, wave 0 stores the header bytes, lane 8c of the round's wave chunk
// c's four CRC bytes, a round's valid pieces tile the packet's full chunks,
// and the ragged path stores the bytes behind them.  No destination byte is
// read.  No store falls outside the stream.  Every load is of bytes of
// [data, data + len) only: 16-B pieces of full chunks and single bytes.  No
// atomics, no cross-workgroup dependence, no spinning.  Without checksums
// (CSUM = false) the same kernel copies and frames and touches no table.
//
// hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S: 62 VGPRs, 102 SGPRs
// (48 / 78 without checksums), 159 776 B of dynamic LDS (32 B without),
// private_segment_fixed_size 0, no flat_ or scratch_ instruction; the waits
// the compiler chose are written up in DESIGN.md section 16.
#include "crc32c_outpkt.h"
#include "wire_fused_crc.h"
#include "wire_fused_internal.h"

namespace hdfs_wire_fused {

namespace {

using hdfs_wire::kChunk;
using hdfs_wire::packet_at;

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

// The wave's round of packet i: everything here is wave-uniform.  i >= npk
// (past the workgroup's last packet) is a round of nothing: every range empty.
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
// stores byte t.
FUSED_DEV void header(uint32_t *hdr, const Write &w, const Unit &u, uint32_t lane) {
  if (lane == 0u)
    hdfs_crc32c::outpkt::put_out_header(reinterpret_cast<uint8_t *>(hdr), int(w.proto), u.p.off, u.p.seq,
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

// The packet's chunk shorter than 512 B (n bytes behind its full chunks, n =
// 0: none), by one whole wave: copied, and its CRC stored.  Byte f of the zero
// frame holds byte f - pad of the chunk; below pad the offset wraps out of the
// range.
template <bool CSUM>
FUSED_DEV void ragged_chunk(const uint32_t *img, const uint32_t *tab, const Write &w, const Unit &u, uint32_t lane) {
  const uint32_t nfull = u.p.dlen / kChunk, n = u.p.dlen % kChunk, pad = kChunk - n;
  const __amdgpu_buffer_rsrc_t rs =
      range_of(reinterpret_cast<uintptr_t>(w.data) + u.p.data_off + uintptr_t(kChunk) * nfull, n);
  const __amdgpu_buffer_rsrc_t rd = range_of(u.d0 + uintptr_t(kChunk) * nfull, n);
  uint32_t b[8];
#pragma unroll
  for (uint32_t j = 0; j < 8; j++) b[j] = load8(rs, 8u * lane + j - pad);
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

}  // namespace

template <bool CSUM>
__global__ __launch_bounds__(1024) void frame_fused_kernel(Write w, const uint32_t *__restrict__ tab) {
  extern __shared__ uint32_t lds[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  uint32_t *hdr = lds;
  uint32_t init512 = 0u;
  if (CSUM) {
    hdr = lds + crc::kImageWords;
    // the image: thread t replicates slicing entry t 32 times (eight 16-B writes), then the Z tables as they are
    const uint32_t v = tab[crc::kCompactSlice + tid];
    u32x4 *p = reinterpret_cast<u32x4 *>(lds + crc::slice_at(tid >> 8, tid & 255u, 0u));
#pragma unroll
    for (int j = 0; j < 8; j++) p[j] = u32x4{v, v, v, v};
#pragma unroll
    for (uint32_t j = 0; j < 7; j++) lds[crc::kImageZ + 1024u * j + tid] = tab[crc::kCompactZ + 1024u * j + tid];
    init512 = tab[crc::kCompactInit + kChunk];
    __syncthreads();
  }
  const uint32_t lo = 64u * (lane & 15u) + 16u * (lane >> 4);
  const uint32_t G = gridDim.x;
  uint32_t i = blockIdx.x;
  // Two register sets take turns (the loop is unrolled twice by hand): a copy
  // of the next round's registers into the current ones at the loop's end
  // would wait for the loads just issued.
  u32x4 ra[4], rb[4];
  Unit u = unit_of(w, i, wave);
  load_round(ra, u, lo);
  auto step = [&](const u32x4(&cur)[4], u32x4(&nxt)[4]) {
    const Unit un = unit_of(w, i + G, wave);  // i + G < 2^32: npk < 2^25, G <= kMaxGroups
    load_round(nxt, un, lo);                  // the next packet's loads, ahead of this round's stores
    store_round(cur, u, lo);
    crc_round<CSUM>(lds, cur, u, wave, lane, init512);
    if (wave == 0u) {
      header(hdr, w, u, lane);
      ragged_chunk<CSUM>(lds, tab, w, u, lane);
    }
    i += G;
    u = un;
  };
  while (i < w.npk) {
    step(ra, rb);
    if (i >= w.npk) break;
    step(rb, ra);
  }
}

hipError_t prepare_frame_fused() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&frame_fused_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kHdrWords) * sizeof(uint32_t)));
}

hipError_t launch_frame_fused(const Write &w, const uint32_t *tab, uint32_t groups, hipStream_t stream) {
  if (!w.npk) return hipSuccess;
  if (!groups || groups > kMaxGroups || w.hb > 4u * kHdrWords - 1u || (w.csum && !tab)) return hipErrorInvalidValue;
  if (w.csum)
    hipLaunchKernelGGL(frame_fused_kernel<true>, dim3(groups), dim3(64 * kWaves),
                       (crc::kImageWords + kHdrWords) * sizeof(uint32_t), stream, w, tab);
  else
    hipLaunchKernelGGL(frame_fused_kernel<false>, dim3(groups), dim3(64 * kWaves), kHdrWords * sizeof(uint32_t),
                       stream, w, tab);
  return hipGetLastError();
}

}  // namespace hdfs_wire_fused
