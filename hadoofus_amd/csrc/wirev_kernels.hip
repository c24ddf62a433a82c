// A write held in a list of device fragments as one wire stream on gfx950:
// frame_gather_kernel, frame_packets_kernel with a fragment table for a data
// source.
//
// Workgroup b serves slice b % slices of packet b / slices, as
// frame_packets_kernel does.  The packet's data [data_off, data_off + dlen)
// of the fragments' concatenation is cut where fragments end: the workgroup
// finds the fragment that holds data_off by binary search of the table's
// `at` column (the k with at[k] <= data_off < at[k + 1]; mid stays inside
// the array), then walks forward, and every piece
//     [max(data_off, at[k]), min(data_off + dlen, at[k + 1]))
// is one frame::copy_region (wire_frame.h) from base[k] + (piece start -
// at[k]) to the piece's place in the packet's data region: slice 0 stores
// the piece's head and tail bytes, the piece's interior 16-B blocks are
// dealt to the slices.  Slice 0 then copies the CRCs and composes the header
// with frame::frame_crcs_and_header, the code frame_packet runs.
//
// The packet index and so the search, the walk and every piece's bounds are
// uniform across the workgroup, and the table is read through the constant
// address space: scalar loads and a scalar loop, one round trip per piece.
//
// Every byte once: the pieces tile the packet's data region (the table's
// `at` rises strictly and ends at the write's length, which wirev.cpp
// builds and the walk re-checks: it stops at an entry that does not
// continue the one before, and never follows k past nf); a piece's head,
// interior and tail tile the piece; heads and tails are slice 0's alone, so
// two pieces that meet inside one 16-B block of the stream are both
// byte-stored by slice 0.  No destination byte is read, no store falls
// outside the packet, no atomics, no waiting on other workgroups, no
// spinning.  Every dword loaded holds a byte of its piece's source
// (copy_region), so loads stay inside the aligned dwords of the fragment.
#include "crc32c_outpkt.h"
#include "wire_frame.h"
#include "wirev_internal.h"

namespace hdfs_wirev {

using hdfs_wire::Pkt;
using hdfs_wire::Write;
namespace frame = hdfs_wire::frame;

#define CAS __attribute__((address_space(4)))

template <bool SC1>
__global__ __launch_bounds__(256) void frame_gather_kernel(Write w, const CAS Frag *tab, uint32_t nf) {
  __shared__ uint32_t lh[8];
  const uint32_t tid = threadIdx.x;
  const uint32_t i = blockIdx.x / w.slices, slice = blockIdx.x - i * w.slices;
  if (i >= w.npk) return;
  const Pkt p = hdfs_wire::packet_at(w, i);
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(w.wire) + p.wire_off;
  const uintptr_t d0 = h0 + w.hb + 4u * uintptr_t(p.ncrc);
  if (p.dlen && nf) {
    const uint64_t a = p.data_off, b = a + p.dlen;
    // at[lo] <= a < at[hi] throughout: at[0] == 0, at[nf] == w.len > a
    uint32_t lo = 0, hi = nf;
    while (hi - lo > 1u) {
      const uint32_t mid = (lo + hi) >> 1;  // 1 <= mid <= nf - 1
      if (tab[mid].at <= a)
        lo = mid;
      else
        hi = mid;
    }
    uint64_t pos = a;
    for (uint32_t k = lo; k < nf && pos < b; k++) {
      const uint64_t fa = tab[k].at, fe = tab[k + 1].at;  // k + 1 <= nf: the sentinel
      if (fa > pos || fe <= pos) break;                   // not the table wirev.cpp builds: nothing more is stored
      const uint64_t pe = fe < b ? fe : b;
      frame::copy_region<SC1>((frame::gbytes)(tab[k].base + (pos - fa)), d0 + uintptr_t(pos - a),
                              d0 + uintptr_t(pe - a), slice == 0u, slice, w.slices, tid);
      pos = pe;
    }
  }
  if (slice != 0u) return;
  frame::frame_crcs_and_header<SC1>(w, p, h0, lh, tid);
}

hipError_t launch_frame_gather(const Write &w, const Frag *tab, uint32_t nf, bool sc1, hipStream_t stream) {
  if (!w.npk) return hipSuccess;
  if (!w.slices || w.slices > hdfs_wire::kMaxSlices || w.hb > 31u || uint64_t(w.npk) * w.slices > 0x7FFFFFFFull ||
      (w.len && (!nf || !tab)))
    return hipErrorInvalidValue;
  const dim3 grid(w.npk * w.slices);
  if (sc1)
    hipLaunchKernelGGL(frame_gather_kernel<true>, grid, dim3(256), 0, stream, w, (const CAS Frag *)tab, nf);
  else
    hipLaunchKernelGGL(frame_gather_kernel<false>, grid, dim3(256), 0, stream, w, (const CAS Frag *)tab, nf);
  return hipGetLastError();
}

}  // namespace hdfs_wirev
