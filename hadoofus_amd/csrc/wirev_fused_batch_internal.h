// Shared between wirev_fused_batch.cpp (host entry points) and
// wirev_fused_batch_kernels.hip.
#ifndef HADOOFUS_WIREV_FUSED_BATCH_INTERNAL_H
#define HADOOFUS_WIREV_FUSED_BATCH_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_internal.h"
#include "wirev_fused_internal.h"

namespace hdfs_wirev_fused_batch {

using hdfs_wire::Pkt;
using hdfs_wire::Write;  // Write::data, Write::crc and Write::slices are unused here: the data are the fragments'
using hdfs_wirev_fused::Frag;

constexpr uint32_t kBatchMaxGroups = 1024;  // workgroups of one launch

// The device tables of one batch, one allocation, one upload, in an order that
// keeps Frag 16-byte aligned (nw: the writes that have packets, nfe: the
// entries of the fragment table, every write's sentinel included):
//   Frag     ft[nfe]      write after write, each write's non-empty fragments
//                         with `at` rising strictly from 0 inside the write,
//                         then its own sentinel {NULL, len_k}
//   Write    tab[nw]      in batch order: data == NULL, crc == NULL, wire set
//   uint32_t pk0[nw + 1]  pk0[k]: packets of the writes ahead of write k;
//                         pk0[nw]: all of them
//   uint32_t fr0[nw + 1]  fr0[k]: index of write k's first Frag; fr0[nw] == nfe
// The host drops writes without packets, so pk0 rises strictly; a write of
// length 0 with finish has a slice that holds only its sentinel.
struct Tables {
  size_t tab, pk0, fr0, bytes;  // byte offsets from ft, and the whole
};
inline Tables tables_of(size_t nw, size_t nfe) {
  Tables t;
  t.tab = nfe * sizeof(Frag);
  t.pk0 = t.tab + nw * sizeof(Write);
  t.fr0 = t.pk0 + (nw + 1) * sizeof(uint32_t);
  t.bytes = t.fr0 + (nw + 1) * sizeof(uint32_t);
  return t;
}
static_assert(sizeof(Frag) % alignof(Write) == 0 && sizeof(Write) % sizeof(uint64_t) == 0,
              "the tables behind the fragments are aligned");

// Once per device, before the first launch there: the kernel's LDS (the table
// image, more than 64 KiB) is allowed.
hipError_t prepare_frame_fused_gather_batch();

// Writes every stream of the nw writes of the tables at `tables` (device,
// tables_of(nw, nfe)), chunk CRCs included (csum): `groups` workgroups of 1024
// (1 <= groups <= kBatchMaxGroups), workgroup b taking global packets b, b +
// groups, ... of the batch.  1 <= nw <= total_pk == pk0[nw]; every entry's hb,
// proto and csum are the batch's.  crc_tab: the compact tables
// (wire_fused_crc.h) of the batch's polynomial in device memory; unused
// without csum.
hipError_t launch_frame_fused_gather_batch(const void *tables, uint32_t nw, uint32_t nfe, uint32_t total_pk,
                                           uint32_t proto, bool csum, const uint32_t *crc_tab, uint32_t groups,
                                           hipStream_t stream);

}  // namespace hdfs_wirev_fused_batch

#endif  // HADOOFUS_WIREV_FUSED_BATCH_INTERNAL_H
