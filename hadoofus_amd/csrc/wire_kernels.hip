// A write's packets as one wire stream on gfx950: frame_packets_kernel, the
// inverse of packet_gather_kernel / copy_pieces_kernel of the main library.
//
// Workgroup b serves slice b % slices of packet b / slices.  What it does
// with that packet -- the three regions, the cut at the destination's 16-B
// grid, the funnel-shifted windows, the pipelined interior, the header
// composed into LDS -- is frame::frame_packet (wire_frame.h), shared with the
// batch library's kernel.
//
// Every byte of [wire, wire + wire_len) is stored exactly once: the packets
// tile the stream (wire_layout.h checks that on the host) and frame_packet
// stores every byte of its packet once.  No destination byte is read, nothing
// outside the stream is stored.  No atomics, no waiting on other workgroups;
// LDS holds the 31 header bytes.
#include "crc32c_outpkt.h"
#include "wire_frame.h"
#include "wire_internal.h"

namespace hdfs_wire {

template <bool SC1>
__global__ __launch_bounds__(256) void frame_packets_kernel(Write w) {
  __shared__ uint32_t lh[8];
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x / w.slices, slice = blockIdx.x - i * w.slices;
  if (i >= w.npk) return;
  frame::frame_packet<SC1>(w, i, slice, w.slices, lh, tid);
}

hipError_t launch_frame_packets(const Write &w, bool sc1, hipStream_t stream) {
  if (!w.npk) return hipSuccess;
  if (!w.slices || w.slices > kMaxSlices || w.hb > 31u || uint64_t(w.npk) * w.slices > 0x7FFFFFFFull)
    return hipErrorInvalidValue;
  const dim3 grid(w.npk * w.slices);
  if (sc1)
    hipLaunchKernelGGL(frame_packets_kernel<true>, grid, dim3(256), 0, stream, w);
  else
    hipLaunchKernelGGL(frame_packets_kernel<false>, grid, dim3(256), 0, stream, w);
  return hipGetLastError();
}

}  // namespace hdfs_wire
