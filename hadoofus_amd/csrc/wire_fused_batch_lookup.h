// The write a global packet index belongs to, written once for host and
// device: frame_fused_batch_kernel (wire_fused_batch_kernels.hip) runs it on
// the prefix array in device memory, through the constant address space, so on
// the scalar unit; tests/consumer/wire_fused_batch_selftest.cpp runs the same
// function on the same array in host memory against a linear scan.  No HIP
// header is needed to compile it.
//
// pk0[0 .. nw] rises strictly from 0 (the host drops writes without packets):
// pk0[k] is the number of packets of the writes ahead of write k, pk0[nw] all
// of them.  For g < pk0[nw] there is one k with pk0[k] <= g < pk0[k + 1].
//
// A workgroup walks g = b, b + G, b + 2G, ..., so g only grows and the write
// found last is a lower bound of the next answer (hint).  From the hint the
// function hops forward at most kLookupHops entries, one load each: writes of
// many packets answer on the first.  Past the hops it bounds the answer from
// above: every write has a packet, so pk0[hint + d] >= pk0[hint] + d and the
// answer is at most hint + (g - pk0[hint]).  That entry is probed first -- it
// is the answer whenever every write between has one packet, the case of many
// tiny writes -- and what is left is binary-searched.  A step therefore costs
// at most kLookupHops + 1 + ceil(log2 min(nw, g - pk0[hint])) dependent loads,
// and never a walk over the entries between.
#ifndef HADOOFUS_WIRE_FUSED_BATCH_LOOKUP_H
#define HADOOFUS_WIRE_FUSED_BATCH_LOOKUP_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_FUSED_BATCH_HD __host__ __device__ inline
#else
#define HDFS_FUSED_BATCH_HD inline
#endif

namespace hdfs_wire_fused {

constexpr uint32_t kLookupHops = 2;

// P: a pointer to const uint32_t in any address space.  Needs hint <= the
// answer and g < pk0[nw]; every index read lies in [hint, nw - 1].
template <class P>
HDFS_FUSED_BATCH_HD uint32_t write_of(P pk0, uint32_t nw, uint32_t g, uint32_t hint) {
  const uint32_t base = pk0[hint];  // <= g; independent of the hops' loads
  uint32_t k = hint;
  for (uint32_t h = 0; h < kLookupHops; h++) {
    if (k + 1u >= nw || g < pk0[k + 1u]) return k;  // pk0[nw] > g needs no load
    k++;
  }
  // pk0[k] <= g: every hop saw it.  The answer is at most top.
  const uint32_t reach = g - base;  // < 2^29
  const uint32_t top = reach < nw - 1u - hint ? hint + reach : nw - 1u;
  if (top <= k || pk0[top] <= g) return top;
  // pk0[lo] <= g < pk0[hi] throughout
  uint32_t lo = k, hi = top;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);  // lo < mid < hi
    if (pk0[mid] <= g)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_BATCH_LOOKUP_H
