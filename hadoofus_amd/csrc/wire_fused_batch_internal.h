// Shared between wire_fused_batch.cpp (host entry points) and
// wire_fused_batch_kernels.hip.
#ifndef HADOOFUS_WIRE_FUSED_BATCH_INTERNAL_H
#define HADOOFUS_WIRE_FUSED_BATCH_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_internal.h"

namespace hdfs_wire_fused {

using hdfs_wire::Pkt;
using hdfs_wire::Write;  // Write::crc and Write::slices are unused here: there is no CRC array

constexpr uint32_t kBatchMaxGroups = 1024;  // workgroups of one launch

// The device tables of one batch, one allocation, one upload (the shape of
// wire_batch_internal.h's):
//   Write    tab[nw]      the writes that have packets, in batch order, data
//                         and wire set
//   uint32_t pk0[nw + 1]  pk0[k]: packets of the writes ahead of write k;
//                         pk0[nw]: all of them
// The host drops writes without packets, so pk0 rises strictly and write_of
// (wire_fused_batch_lookup.h) has one answer.
inline size_t fused_batch_table_bytes(size_t nw) { return nw * sizeof(Write) + (nw + 1) * sizeof(uint32_t); }
static_assert(sizeof(Write) % sizeof(uint64_t) == 0, "pk0 behind the table is aligned");

// Once per device, before the first launch there: the kernel's LDS (the table
// image, more than 64 KiB) is allowed.
hipError_t prepare_frame_fused_batch();

// Writes every stream of the nw writes of the tables at tab, chunk CRCs
// included (csum): `groups` workgroups of 1024 (1 <= groups <=
// kBatchMaxGroups), workgroup b taking global packets b, b + groups, ... of
// the batch.  1 <= nw <= total_pk == pk0[nw]; every entry's hb, proto and csum
// are the batch's.  crc_tab: the compact tables (wire_fused_crc.h) of the
// batch's polynomial in device memory; unused without csum.
hipError_t launch_frame_fused_batch(const void *tab, uint32_t nw, uint32_t total_pk, uint32_t proto, bool csum,
                                    const uint32_t *crc_tab, uint32_t groups, hipStream_t stream);

}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_BATCH_INTERNAL_H
