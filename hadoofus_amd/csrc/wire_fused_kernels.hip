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
// The round's device code is wire_fused_round.h's, shared with
// frame_fused_batch_kernel (wire_fused_batch_kernels.hip).
//
// hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S: 62 VGPRs, 102 SGPRs
// (48 / 78 without checksums), 159 776 B of dynamic LDS (32 B without),
// private_segment_fixed_size 0, no flat_ or scratch_ instruction; the waits
// the compiler chose are written up in DESIGN.md section 16.
#include "wire_fused_internal.h"
#include "wire_fused_round.h"

namespace hdfs_wire_fused {

template <bool CSUM>
__global__ __launch_bounds__(1024) void frame_fused_kernel(Write w, const uint32_t *__restrict__ tab) {
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
      header(hdr, w.proto, u, lane);
      ragged_chunk<CSUM>(lds, tab, reinterpret_cast<uintptr_t>(w.data) + u.p.data_off, u, lane);
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
