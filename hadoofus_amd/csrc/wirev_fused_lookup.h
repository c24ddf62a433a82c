// The fragment a byte of a gather write lies in, and how a write's 4 KiB
// rounds fall over its fragments, written once for host and device:
// frame_fused_gather_kernel (wirev_fused_kernels.hip) runs frag_of on the
// fragment table in device memory, through the constant address space, so on
// the scalar unit; wirev_fused.cpp runs frag_of and count_packet on the same
// offsets in host memory for hdfs_wirev_fused_layout; and
// tests/consumer/wirev_fused_selftest.cpp runs both against a linear scan and a
// brute-force model.  No HIP header is needed to compile it.
//
// at[0 .. nf] rises strictly from 0 (the host drops empty fragments): at[k] is
// the first byte of fragment k in the fragments' concatenation, at[nf] the
// write's length.  For pos < at[nf] there is one k with at[k] <= pos <
// at[k + 1].
//
// A wave walks round v of packets b, b + G, b + 2G, ..., so pos only grows and
// the fragment found last is a lower bound of the next answer (hint).  From
// the hint the function hops forward at most kFragHops entries, one load each:
// fragments of many rounds answer on the first.  Past the hops it bounds the
// answer from above: every fragment has a byte, so at[hint + d] >= at[hint] +
// d and the answer is at most hint + (pos - at[hint]).  That entry is probed
// first -- it is the answer whenever every fragment between has one byte --
// and what is left is binary-searched.  A lookup therefore costs at most
// kFragHops + 2 + ceil(log2 min(nf, pos - at[hint])) dependent loads, and
// never a walk over the entries between.
#ifndef HADOOFUS_WIREV_FUSED_LOOKUP_H
#define HADOOFUS_WIREV_FUSED_LOOKUP_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_WIREV_FUSED_HD __host__ __device__ inline
#else
#define HDFS_WIREV_FUSED_HD inline
#endif

namespace hdfs_wirev_fused {

constexpr uint32_t kFragHops = 2;
constexpr uint32_t kLookupChunk = 512, kLookupRound = 4096;  // wire_internal.h's kChunk, wire_fused_round.h's kRound

// A: anything whose at[k] is the uint64_t offset of entry k (a pointer to
// const uint64_t; the kernel's view of its table's `at` column).  Needs
// at[hint] <= pos < at[nf]; every index read lies in [hint, nf - 1].
template <class A>
HDFS_WIREV_FUSED_HD uint32_t frag_of(A at, uint32_t nf, uint64_t pos, uint32_t hint) {
  const uint64_t base = at[hint];  // <= pos; independent of the hops' loads
  uint32_t k = hint;
  for (uint32_t h = 0; h < kFragHops; h++) {
    if (k + 1u >= nf || pos < at[k + 1u]) return k;  // at[nf] > pos needs no load
    k++;
  }
  // at[k] <= pos: every hop saw it.  The answer is at most top.
  const uint64_t reach = pos - base;
  const uint32_t top = reach < uint64_t(nf - 1u - hint) ? hint + uint32_t(reach) : nf - 1u;
  if (top <= k || at[top] <= pos) return top;
  // at[lo] <= pos < at[hi] throughout
  uint32_t lo = k, hi = top;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + ((hi - lo) >> 1);  // lo < mid < hi
    if (at[mid] <= pos)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// What hdfs_wirev_fused_layout reports about the kernel's paths.
struct RoundCounts {
  uint64_t rounds = 0;         // 4 KiB rounds with at least one full chunk
  uint64_t seamed_rounds = 0;  // those whose full chunks do not lie inside one fragment
  uint64_t seamed_ragged = 0;  // chunks shorter than 512 B that do not
  uint32_t max_frags_per_round = 0;  // most fragments under one round's full chunks
};

// Fragments that hold bytes of [a, e) (a < e <= at[nf]), the first of them
// k = frag_of(a): one load each.
template <class A>
HDFS_WIREV_FUSED_HD uint32_t frags_under(A at, uint32_t k, uint64_t e) {
  uint32_t n = 1;
  while (at[k + n] < e) n++;  // at[k + n] < e <= at[nf]: k + n < nf
  return n;
}

// One packet's data [a, a + dlen) of the write, as the kernel cuts it: rounds
// of eight full chunks from a, then the chunk shorter than 512 B.  Packets are
// given in stream order, hint carried from one to the next (0 at first).
template <class A>
HDFS_WIREV_FUSED_HD void count_packet(A at, uint32_t nf, uint64_t a, uint32_t dlen, uint32_t &hint, RoundCounts &c) {
  const uint64_t full = uint64_t(dlen / kLookupChunk) * kLookupChunk;
  for (uint64_t r = 0; r < full; r += kLookupRound) {
    const uint64_t ra = a + r, re = a + (full - r < kLookupRound ? full : r + kLookupRound);
    hint = frag_of(at, nf, ra, hint);
    const uint32_t n = frags_under(at, hint, re);
    c.rounds++;
    c.seamed_rounds += n > 1u ? 1u : 0u;
    if (n > c.max_frags_per_round) c.max_frags_per_round = n;
  }
  if (dlen % kLookupChunk) {
    hint = frag_of(at, nf, a + full, hint);
    c.seamed_ragged += frags_under(at, hint, a + dlen) > 1u ? 1u : 0u;
  }
}

}  // namespace hdfs_wirev_fused

#endif  // HADOOFUS_WIREV_FUSED_LOOKUP_H
