// What connects the two lookups of a batch of gather writes, written once for
// host and device: frame_fused_gather_batch_kernel
// (wirev_fused_batch_kernels.hip) runs it on the tables in device memory,
// through the constant address space, so on the scalar unit;
// tests/consumer/wirev_fused_batch_selftest.cpp runs the same code on the same
// tables in host memory against a brute-force model.  No HIP header is needed
// to compile it.
//
// The tables (wirev_fused_batch_internal.h):
//   pk0[0 .. nw]  the packet prefix of the writes that have packets, rising
//                 strictly from 0 (write_of, wire_fused_batch_lookup.h)
//   fr0[0 .. nw]  fr0[k]: the index of write k's first entry in the fragment
//                 table; its slice is entries [fr0[k], fr0[k + 1]): the
//                 write's nf_k = fr0[k + 1] - fr0[k] - 1 non-empty fragments,
//                 `at` rising strictly from 0 inside the slice, then the
//                 write's own sentinel {NULL, len_k}
// frag_of (wirev_fused_lookup.h) is given one slice and reads [hint, nf_k - 1]
// of it, so the three rules below are what keeps it inside that slice.
//
//   1. The fragment hint belongs to one write.  A wave keeps it from packet to
//      packet only while write_of returns the same write (inside one write the
//      wave's round starts further on every time, so the fragment found last
//      is a lower bound).  When the write changes the hint is 0 again
//      (seek_write).  A hint left from a write of many fragments would
//      otherwise index past a slice of one.
//   2. A global packet at or past the batch's last looks up no write; a round
//      without a full chunk looks up no fragment and no slice (the caller asks
//      slice_of and seek_frag only under u.nfr != 0).  The cursor stays.
//   3. The chunk shorter than 512 B belongs to the current packet, the loads
//      to the next: the kernel issues the next packet's loads, and so runs the
//      next packet's lookups, ahead of the current packet's stores.  The
//      cursor is therefore copied when a packet's lookups are done (`kc` in
//      the kernel) and the ragged chunk gets that copy: its write, whose slice
//      is re-derived from fr0 (two scalar loads by wave 0 instead of three
//      more registers carried by every wave), and its hint.
#ifndef HADOOFUS_WIREV_FUSED_BATCH_LOOKUP_H
#define HADOOFUS_WIREV_FUSED_BATCH_LOOKUP_H

#include <stdint.h>

#include "wire_fused_batch_lookup.h"
#include "wirev_fused_lookup.h"

namespace hdfs_wirev_fused_batch {

using hdfs_wire_fused::write_of;
using hdfs_wirev_fused::frag_of;

// What a wave carries from one global packet to the next.
struct Cursor {
  uint32_t kw = 0;  // the write found last: a lower bound of the next one
  uint32_t kf = 0;  // the fragment found last inside that write's slice: a lower bound of the next one there
};

// A write's slice of the fragment table.
struct Slice {
  uint32_t first;  // index of its first entry
  uint32_t nf;     // its non-empty fragments; entry first + nf is the sentinel
};

// The write of global packet g (g < total == pk0[nw] only; otherwise nothing
// is looked up and the cursor stays).  -> whether g is a packet.
template <class P>
HDFS_WIREV_FUSED_HD bool seek_write(P pk0, uint32_t nw, uint32_t total, uint32_t g, Cursor &c) {
  if (g >= total) return false;
  const uint32_t k = write_of(pk0, nw, g, c.kw);
  if (k != c.kw) c.kf = 0u;  // rule 1
  c.kw = k;
  return true;
}

template <class P>
HDFS_WIREV_FUSED_HD Slice slice_of(P fr0, uint32_t kw) {
  const uint32_t first = fr0[kw];
  return Slice{first, fr0[kw + 1u] - first - 1u};
}

// The fragment of byte pos of the cursor's write (pos < its length); at: the
// `at` column of that write's slice, entry 0 its first fragment.
template <class A>
HDFS_WIREV_FUSED_HD uint32_t seek_frag(A at, uint32_t nf, uint64_t pos, Cursor &c) {
  c.kf = frag_of(at, nf, pos, c.kf);
  return c.kf;
}

}  // namespace hdfs_wirev_fused_batch

#endif  // HADOOFUS_WIREV_FUSED_BATCH_LOOKUP_H
