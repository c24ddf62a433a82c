// Shared between wirev_fused.cpp (host entry points) and
// wirev_fused_kernels.hip, whose gather-only device helpers are at the end
// (seen only by a file that has included wire_fused_round.h).
#ifndef HADOOFUS_WIREV_FUSED_INTERNAL_H
#define HADOOFUS_WIREV_FUSED_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_internal.h"
#include "wirev_fused_lookup.h"

namespace hdfs_wirev_fused {

using hdfs_wire::Pkt;
using hdfs_wire::Write;  // Write::data, Write::crc and Write::slices are unused here: the data are the fragments'

constexpr uint32_t kMaxGroups = 1024;  // workgroups of one launch

// One non-empty fragment of the write, as in wirev_internal.h: its bytes lie
// at base, the first of them is byte `at` of the fragments' concatenation.
// The table holds the nf fragments in order, `at` rising strictly from 0, and
// one sentinel behind them, {NULL, len}: fragment k is bytes [at[k], at[k + 1])
// of the write.
struct Frag {
  const uint8_t *base;
  uint64_t at;
};
static_assert(sizeof(Frag) == 16, "Frag layout");

// Once per device, before the first launch there: the kernel's LDS (the table
// image, more than 64 KiB) is allowed.
hipError_t prepare_frame_fused_gather();

// Writes wire[0, wire_len) of write w, chunk CRCs included: `groups`
// workgroups of 1024 (1 <= groups <= kMaxGroups), workgroup b taking packets
// b, b + groups, ...  ft: device Frag[nf + 1].  tab: the compact tables
// (wire_fused_crc.h) of the write's polynomial in device memory; unused
// without csum.
hipError_t launch_frame_fused_gather(const Write &w, const Frag *ft, uint32_t nf, const uint32_t *tab,
                                     uint32_t groups, hipStream_t stream);

}  // namespace hdfs_wirev_fused

// ---- device: a round and a ragged chunk whose bytes lie in several fragments ----
#ifdef HADOOFUS_WIRE_FUSED_ROUND_H

namespace hdfs_wirev_fused {

using namespace hdfs_wire_fused;  // the round: wire_fused_round.h's

#define CAS __attribute__((address_space(4)))

// The table through the constant address space (scalar loads), and its `at`
// column as frag_of wants it.
typedef const CAS Frag *FragTab;
struct AtOf {
  FragTab t;
  __device__ __forceinline__ uint64_t operator[](uint32_t k) const { return t[k].at; }
};

// Lane piece q (16 B at 16 q of the round) holds a byte of the piece [ps, pe)
// of the round without lying inside it: its owner (the lane whose lo it is)
// loads it byte by byte through r, the range of exactly the piece, whose byte
// 0 is byte ps of the round.  Outside the piece the offset wraps out of the
// range, so those bytes stay zero.  q is uniform, so is the register it goes to.
FUSED_DEV void edge_piece(u32x4 (&v)[4], __amdgpu_buffer_rsrc_t r, uint32_t q, uint32_t ps, uint32_t lo) {
  const uint32_t o = 16u * q;
  const bool mine = (o & 1023u) == lo;
  uint32_t d[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (uint32_t b = 0; b < 16; b++) d[b >> 2] |= load8(r, mine ? o + b - ps : kNowhere) << (8u * (b & 3u));
  const u32x4 e = u32x4{d[0], d[1], d[2], d[3]};
  const uint32_t j = q >> 6;
#pragma unroll
  for (uint32_t jj = 0; jj < 4; jj++) v[jj] |= e & (0u - uint32_t(jj == j));  // a mask, not an index: registers
}

// The seamed load of a round: v holds zeros (load_round through an empty
// range); afterwards it holds exactly what load_round would have loaded had
// the round's `bytes` bytes, which start at byte ra of the write in fragment
// k, been contiguous.  A scalar loop over the fragment pieces under the
// round: per piece a range over exactly the piece, one 16-B load per lane
// piece wholly inside it (every other lane piece at kNowhere), the at most two
// lane pieces that hold the piece's first or last byte without lying inside
// it by byte loads, everything OR-ed together.  The loop stops at an entry
// that does not continue the one before and never follows k past nf.
FUSED_DEV void seam_round(u32x4 (&v)[4], FragTab ft, uint32_t nf, uint32_t k, uint64_t ra, uint32_t bytes,
                          uint32_t lo) {
  uint32_t ps = 0u;  // the piece's first byte in the round
  for (; k < nf && ps < bytes; k++) {
    const uint64_t fa = ft[k].at, fe = ft[k + 1u].at, pos = ra + ps;  // k + 1 <= nf: the sentinel
    if (fa > pos || fe <= pos) break;  // not the table wirev_fused.cpp builds: nothing more is loaded
    const uint64_t left = fe - pos;
    const uint32_t pe = left < uint64_t(bytes - ps) ? ps + uint32_t(left) : bytes;
    const __amdgpu_buffer_rsrc_t r = range_of(reinterpret_cast<uintptr_t>(ft[k].base) + uintptr_t(pos - fa), pe - ps);
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
      const uint32_t o = lo + 1024u * j;
      v[j] |= load16(r, (o >= ps && o + 16u <= pe) ? o - ps : kNowhere);
    }
    const uint32_t q0 = ps >> 4, q1 = (pe - 1u) >> 4;  // the lane pieces of the piece's first and last byte
    if ((ps & 15u) || pe < 16u * q0 + 16u) edge_piece(v, r, q0, ps, lo);
    if (q1 != q0 && (pe & 15u)) edge_piece(v, r, q1, ps, lo);
    ps = pe;
  }
}

// ragged_chunk for a chunk whose n bytes start at byte ca of the write, in or
// behind fragment `hint`: the same loop of pieces, byte loads OR-ed into the
// zero frame; copy and CRC are ragged_finish's.
template <bool CSUM>
FUSED_DEV void ragged_gather(const uint32_t *img, const uint32_t *tab, FragTab ft, uint32_t nf, uint32_t hint,
                             const Unit &u, uint32_t lane) {
  const uint32_t nfull = u.p.dlen / kChunk, n = u.p.dlen % kChunk, pad = kChunk - n;
  uint32_t b[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (n && nf) {  // uniform; ca < len, as frag_of needs
    const uint64_t ca = u.p.data_off + uint64_t(kChunk) * nfull;
    uint32_t ps = 0u;
    for (uint32_t k = frag_of(AtOf{ft}, nf, ca, hint); k < nf && ps < n; k++) {
      const uint64_t fa = ft[k].at, fe = ft[k + 1u].at, pos = ca + ps;
      if (fa > pos || fe <= pos) break;
      const uint64_t left = fe - pos;
      const uint32_t pe = left < uint64_t(n - ps) ? ps + uint32_t(left) : n;
      const __amdgpu_buffer_rsrc_t r = range_of(reinterpret_cast<uintptr_t>(ft[k].base) + uintptr_t(pos - fa), pe - ps);
#pragma unroll
      for (uint32_t j = 0; j < 8; j++) b[j] |= load8(r, 8u * lane + j - pad - ps);
      ps = pe;
    }
  }
  ragged_finish<CSUM>(img, tab, b, u, lane);
}

}  // namespace hdfs_wirev_fused

#endif  // HADOOFUS_WIRE_FUSED_ROUND_H
#endif  // HADOOFUS_WIREV_FUSED_INTERNAL_H
