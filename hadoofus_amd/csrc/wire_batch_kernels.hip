// The packets of a batch of writes as one wire stream per write, in one
// launch on gfx950: frame_batch_kernel.
//
// Workgroup b serves slice b % 4 of global packet g = b / 4, counted over the
// whole batch in batch order.  It finds the write the packet belongs to by
// binary search of the prefix array pk0 (the k with pk0[k] <= g < pk0[k + 1])
// and frames packet g - pk0[k] of write k exactly as frame_packets_kernel
// frames it: frame::frame_packet (wire_frame.h), the one definition.
//
// Writes without packets (empty, no finish) are dropped on the host
// (wire_batch.cpp), not skipped here: the table holds only writes with at
// least one packet, so pk0 rises strictly and no entry with zero packets can
// be selected.
//
// g is uniform across the workgroup, and the tables are read through the
// constant address space, as the main library reads its SegDev table: the
// search and the load of the entry are scalar loads (s_load_*) and a scalar
// loop, the entry sits in SGPRs as frame_packets_kernel's kernel argument
// does.  Plain stores, no atomics, no waiting on other workgroups, no
// spinning, no destination byte read.
#include "crc32c_outpkt.h"
#include "wire_batch_internal.h"
#include "wire_frame.h"

namespace hdfs_wire {

#define CAS __attribute__((address_space(4)))

__global__ __launch_bounds__(256) void frame_batch_kernel(const CAS Write *tab, const CAS uint32_t *pk0, uint32_t nw,
                                                          uint32_t total_pk) {
  __shared__ uint32_t lh[8];
  const uint32_t g = blockIdx.x / kBatchSlices, slice = blockIdx.x % kBatchSlices;
  if (g >= total_pk) return;
  // pk0[lo] <= g < pk0[hi] throughout: pk0[0] == 0, pk0[nw] == total_pk
  uint32_t lo = 0, hi = nw;
  while (hi - lo > 1u) {
    const uint32_t mid = (lo + hi) >> 1;  // 1 <= mid <= nw - 1
    if (pk0[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  const CAS Write *p = tab + lo;
  const Write w{p->data, p->crc, p->wire, p->len, p->off, p->seq, p->n0, p->npk, p->hb, p->proto, p->csum, p->finish,
                p->slices};
  const uint32_t i = g - pk0[lo];
  if (i >= w.npk) return;
  frame::frame_packet<false>(w, i, slice, kBatchSlices, lh, threadIdx.x);
}

hipError_t launch_frame_batch(const void *tab, uint32_t nw, uint32_t total_pk, hipStream_t stream) {
  if (!total_pk) return hipSuccess;
  if (!nw || nw > total_pk || uint64_t(total_pk) * kBatchSlices > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const Write *t = static_cast<const Write *>(tab);
  const uint32_t *pk0 = reinterpret_cast<const uint32_t *>(t + nw);
  hipLaunchKernelGGL(frame_batch_kernel, dim3(total_pk * kBatchSlices), dim3(256), 0, stream, (const CAS Write *)t,
                     (const CAS uint32_t *)pk0, nw, total_pk);
  return hipGetLastError();
}

}  // namespace hdfs_wire
