// How the bytes of a scatter read fall over its destination fragments,
// written once for host and device: unframe_scatter_batch_kernel
// (preadv_batch_kernels.hip) runs it on the tables in device memory, through
// the constant address space, so on the scalar unit;
// tests/consumer/preadv_batch_selftest.cpp runs the same code on the same
// tables in host memory against a per-byte brute-force model.  No HIP header is
// needed to compile it.  It is the store-side twin of seam_round
// (wirev_fused_internal.h): there a round's registers are gathered from the
// fragments under it, here they are scattered over them.
//
// The tables (preadv_batch_internal.h):
//   fr0[0 .. n]   by ENTRY of the batch, not by slot (the probe deals the slots
//                 on the device, the host lays the fragments): fr0[e] is the
//                 index of entry e's first row in the fragment table; its slice
//                 is rows [fr0[e], fr0[e + 1]): the entry's nf = fr0[e + 1] -
//                 fr0[e] - 1 non-empty fragments, `at` rising strictly from 0
//                 inside the slice, then the entry's own sentinel {NULL, cap}
// Destination position y of an entry (y = payload position - c_begin, 0 <= y <
// read_len <= cap = at[nf]) lies in the one fragment k with at[k] <= y <
// at[k + 1], at byte y - at[k] of it.
//
// A CUT is the part of a wave's unit of work -- a round of up to 4 096 bytes
// of full chunks, or the chunk shorter than 512 B -- that the read's window
// keeps: bytes [sa, sb) of the unit, the first of them at destination position
// y0.  Its PIECES are its intersections with the fragments, in order
// (next_piece): piece [ps, pe) of the unit lies in fragment k from byte foff
// on, and every store of it goes through a range over exactly those pe - ps
// bytes.  In a round, lane piece q is the 16 bytes [16 q, 16 q + 16) one lane
// holds in a register; against a piece it is stored whole (whole_at), byte by
// byte because it holds the piece's first or last byte without lying inside it
// (head_edge, tail_edge, byte_at), or not at all (kOutside: an offset no range
// holds).  A piece shorter than 16 B inside one lane piece is bytes only.
//
// The cursor's rules:
//   1. The fragment hint belongs to one entry.  A wave keeps it from packet to
//      packet only while the packet's slot stays the same; when the slot
//      changes it is 0 again (seek_slot).  A hint left from an entry of many
//      fragments would otherwise index past a slice of one.
//   2. It is consulted at store time, for the CURRENT packet: the kernel issues
//      the next packet's loads ahead of the current packet's stores, and the
//      next packet may belong to another entry.
//   3. Inside an entry a wave's positions only rise (round v of packets b, b +
//      G, ...), so the fragment found last is a lower bound of the next
//      answer.  Wave 0's chunk shorter than 512 B lies behind its round of the
//      same packet and before its round of the next one.
//   4. A cut of zero bytes looks up nothing: neither the slice nor a fragment
//      (the lookup needs y0 < at[nf]).  The cursor stays.
#ifndef HADOOFUS_PREADV_BATCH_LOOKUP_H
#define HADOOFUS_PREADV_BATCH_LOOKUP_H

#include <stdint.h>

#include "wirev_fused_lookup.h"

namespace hdfs_preadv_batch {

using hdfs_wirev_fused::frag_of;

constexpr uint32_t kOutside = 0x80000000u;  // wire_fused_round.h's kNowhere
constexpr uint32_t kNoEntry = 0xFFFFFFFFu;

// What a wave carries from one packet to the next.
struct Cursor {
  uint32_t slot = kNoEntry;  // the slot the hint belongs to
  uint32_t kf = 0;           // the fragment found last inside that entry's slice
};

// An entry's slice of the fragment table.
struct Slice {
  uint32_t first;  // index of its first row
  uint32_t nf;     // its non-empty fragments; row first + nf is the sentinel
};

// One piece of a cut: bytes [ps, pe) of the unit go to fragment k (of the
// slice) from its byte foff on.
struct Piece {
  uint32_t k, ps, pe;
  uint64_t foff;
};

// Where the next piece starts.
struct Walk {
  uint32_t k;   // its fragment
  uint32_t ps;  // its first byte in the unit
};

HDFS_WIREV_FUSED_HD void seek_slot(Cursor &c, uint32_t slot) {
  if (slot != c.slot) {  // rule 1
    c.slot = slot;
    c.kf = 0u;
  }
}

template <class P>
HDFS_WIREV_FUSED_HD Slice slice_of(P fr0, uint32_t entry) {
  const uint32_t first = fr0[entry];
  return Slice{first, fr0[entry + 1u] - first - 1u};
}

// The fragment of destination position y0 of the cursor's entry (y0 < at[nf]);
// at: the `at` column of that entry's slice, row 0 its first fragment.
template <class A>
HDFS_WIREV_FUSED_HD uint32_t seek_frag(A at, uint32_t nf, uint64_t y0, Cursor &c) {
  c.kf = frag_of(at, nf, y0, c.kf);
  return c.kf;
}

// The cut [sa, sb) of the unit, sa at destination position y0 in fragment k, is
// the whole unit of n bytes and lies inside that fragment: no piece walk.
template <class A>
HDFS_WIREV_FUSED_HD bool unseamed(A at, uint32_t k, uint64_t y0, uint32_t sa, uint32_t sb, uint32_t n) {
  return sa == 0u && sb == n && y0 + n <= at[k + 1u];
}

// The next piece of the cut [sa, sb) of the unit, sa at destination position
// y0: w starts at {the fragment of y0, sa}.  -> whether there is one.  Reads
// at[w.k] and at[w.k + 1] only, w.k < nf: rows of the slice, the sentinel the
// last.  The walk ends when the cut does (sb - sa <= at[nf] - y0, so at or
// before the sentinel), and at a row that does not continue the one before:
// not the table the host builds, and nothing more is stored.
template <class A>
HDFS_WIREV_FUSED_HD bool next_piece(A at, uint32_t nf, uint64_t y0, uint32_t sa, uint32_t sb, Walk &w, Piece &p) {
  if (w.ps >= sb || w.k >= nf) return false;
  const uint64_t fa = at[w.k], fe = at[w.k + 1u], pos = y0 + (w.ps - sa);
  if (fa > pos || fe <= pos) return false;
  const uint64_t left = fe - pos;
  const uint32_t pe = left < uint64_t(sb - w.ps) ? w.ps + uint32_t(left) : sb;
  p = Piece{w.k, w.ps, pe, pos - fa};
  w.k++;
  w.ps = pe;
  return true;
}

// A lane's 16 bytes [o, o + 16) of the round against the piece [ps, pe): the
// offset of its 16-B store in the piece's range, or kOutside when it does not
// lie wholly inside.
HDFS_WIREV_FUSED_HD uint32_t whole_at(uint32_t o, uint32_t ps, uint32_t pe) {
  return o >= ps && o + 16u <= pe ? o - ps : kOutside;
}

// Byte `at` of the unit against the piece: its offset in the piece's range, or
// kOutside.
HDFS_WIREV_FUSED_HD uint32_t byte_at(uint32_t at, uint32_t ps, uint32_t pe) {
  return at >= ps && at < pe ? at - ps : kOutside;
}

// The lane piece q that holds the piece's first byte without lying inside it.
HDFS_WIREV_FUSED_HD bool head_edge(uint32_t ps, uint32_t pe, uint32_t &q) {
  q = ps >> 4;
  return (ps & 15u) != 0u || pe < 16u * q + 16u;
}

// The lane piece q that holds the piece's last byte without lying inside it
// and is not head_edge's.
HDFS_WIREV_FUSED_HD bool tail_edge(uint32_t ps, uint32_t pe, uint32_t &q) {
  q = (pe - 1u) >> 4;
  return q != (ps >> 4) && (pe & 15u) != 0u;
}

}  // namespace hdfs_preadv_batch

#endif  // HADOOFUS_PREADV_BATCH_LOOKUP_H
