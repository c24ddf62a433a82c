// A write held in a list of device fragments as one wire stream on gfx950 in
// ONE pass over the data: frame_fused_gather_kernel, frame_fused_kernel
// (wire_fused_kernels.hip) with a fragment table for a data source (DESIGN.md
// section 18).
//
// The grid, the walk and the round are frame_fused_kernel's, the round the
// one definition of wire_fused_round.h: min(CUs, packets) workgroups of 16
// waves, workgroup b takes packets b, b + G, ..., wave v takes round v (4 KiB,
// eight chunks) of the workgroup's packet -- four coalesced 16-B buffer loads,
// the registers stored straight out (nt), the in-register transpose,
// wire_fused_crc.h's lane arithmetic, lane 8c's CRC store -- and wave 0
// composes and stores the header and does the chunk shorter than 512 B.  The
// table image is filled once per workgroup, behind the only barrier; two
// register sets take turns; the next packet's loads are issued ahead of the
// current round's stores.
//
// The source differs.  The write is created with data == NULL, so unit_of's
// u.src is the round's first byte ra in the fragments' concatenation.  A round
// with a full chunk finds the fragment k with at[k] <= ra < at[k + 1]
// (frag_of, wirev_fused_lookup.h: from the fragment the wave found last, a
// bounded number of hops, the upper-bound probe, then a bounded binary
// search).  ra and every bound are wave-uniform and the table is read through
// the constant address space: scalar loads and a scalar loop.  A round with no
// full chunk looks nothing up (its ra may lie at or past the write's end).
//   * Fast round: its full chunks end inside fragment k.  u.src becomes
//     base[k] + (ra - at[k]) and the round is frame_fused_kernel's.
//   * Seamed round: load_round runs through an empty range (zeros, no memory
//     touched) and seam_round (wirev_fused_internal.h) assembles into the same
//     four registers exactly the bytes the fast path would have loaded, piece
//     by piece; store_round and crc_round then run unchanged, so the stream
//     and the CRCs are the fast path's.
// The chunk shorter than 512 B is ragged_gather's: the same loop of pieces by
// byte loads, then ragged_finish, the second half of ragged_chunk.
//
// Invariants.  Every byte of [wire, wire + wire_len) is stored exactly once,
// as frame_fused_kernel stores it; no destination byte is read; no store falls
// outside the stream.  Every vector load goes through a range over exactly
// the bytes of one fragment it may touch, so only the fragments' own bytes
// are read.  The table is read at indices [0, nf] only.  No atomics, no
// cross-workgroup dependence, no spinning.
//
// hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S: 83 VGPRs, 106 SGPRs
// (60 / 90 without checksums), 159 776 B of dynamic LDS (32 B without),
// private_segment_fixed_size 0, no flat_ or scratch_ instruction; five
// loop-invariant SGPRs live in VGPR lanes with checksums.  The waits the
// compiler chose are written up in DESIGN.md section 18.
#include "wire_fused_round.h"
#include "wirev_fused_internal.h"
#include "wirev_fused_lookup.h"

namespace hdfs_wirev_fused {

// The wave's round of packet i with its source found, and its loads issued
// into v.  k: the fragment the wave found last (a lower bound of this one),
// updated.  Everything but the loads' lane offsets is wave-uniform.
FUSED_DEV Unit load_unit(u32x4 (&v)[4], const Write &w, FragTab ft, uint32_t nf, uint32_t i, uint32_t wave,
                         uint32_t &k, uint32_t lo) {
  Unit u = unit_of(w, i, wave);  // w.data == NULL: u.src is the round's first byte in the write
  const uint64_t ra = u.src;
  bool seamed = false;
  if (u.nfr) {  // ra < len
    k = frag_of(AtOf{ft}, nf, ra, k);
    const uint64_t fa = ft[k].at, fe = ft[k + 1u].at;  // k + 1 <= nf: the sentinel
    seamed = ra + u.nfr * kChunk > fe;
    u.src = reinterpret_cast<uintptr_t>(ft[k].base) + uintptr_t(ra - fa);
  }
  Unit ul = u;
  if (seamed) ul.nfr = 0u;  // an empty range: zeros, nothing read
  load_round(v, ul, lo);
  if (seamed) seam_round(v, ft, nf, k, ra, u.nfr * kChunk, lo);
  return u;
}

template <bool CSUM>
__global__ __launch_bounds__(1024) void frame_fused_gather_kernel(Write w, FragTab ft, uint32_t nf,
                                                                  const uint32_t *__restrict__ tab) {
  extern __shared__ uint32_t lds[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  uint32_t *hdr = lds;
  uint32_t init512 = 0u;
  if (CSUM) {
    hdr = lds + crc::kImageWords;
    fill_image(lds, tab, tid);
    init512 = tab[crc::kCompactInit + kChunk];
    __syncthreads();
  }
  const uint32_t lo = 64u * (lane & 15u) + 16u * (lane >> 4);
  const uint32_t G = gridDim.x;
  uint32_t i = blockIdx.x, k = 0u;
  // Two register sets take turns, as in frame_fused_kernel.
  u32x4 ra[4], rb[4];
  Unit u = load_unit(ra, w, ft, nf, i, wave, k, lo);
  uint32_t kc = k;  // k as the current packet's round left it: no later than the fragment of the packet's chunk shorter than 512 B
  auto step = [&](const u32x4(&cur)[4], u32x4(&nxt)[4]) {
    const Unit un = load_unit(nxt, w, ft, nf, i + G, wave, k, lo);  // the next packet's loads, ahead of this round's stores
    store_round(cur, u, lo);
    crc_round<CSUM>(lds, cur, u, wave, lane, init512);
    if (wave == 0u) {
      header(hdr, w.proto, u, lane);
      ragged_gather<CSUM>(lds, tab, ft, nf, kc, u, lane);
    }
    kc = k;
    i += G;
    u = un;
  };
  while (i < w.npk) {
    step(ra, rb);
    if (i >= w.npk) break;
    step(rb, ra);
  }
}

hipError_t prepare_frame_fused_gather() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&frame_fused_gather_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kHdrWords) * sizeof(uint32_t)));
}

hipError_t launch_frame_fused_gather(const Write &w, const Frag *ft, uint32_t nf, const uint32_t *tab,
                                     uint32_t groups, hipStream_t stream) {
  if (!w.npk) return hipSuccess;
  if (!groups || groups > kMaxGroups || w.hb > 4u * kHdrWords - 1u || (w.csum && !tab) || w.data ||
      (w.len && (!nf || !ft)))
    return hipErrorInvalidValue;
  if (w.csum)
    hipLaunchKernelGGL(frame_fused_gather_kernel<true>, dim3(groups), dim3(64 * kWaves),
                       (crc::kImageWords + kHdrWords) * sizeof(uint32_t), stream, w, (FragTab)ft, nf, tab);
  else
    hipLaunchKernelGGL(frame_fused_gather_kernel<false>, dim3(groups), dim3(64 * kWaves),
                       kHdrWords * sizeof(uint32_t), stream, w, (FragTab)ft, nf, tab);
  return hipGetLastError();
}

}  // namespace hdfs_wirev_fused
