// Shared between wire_fused.cpp (host entry points) and wire_fused_kernels.hip.
#ifndef HADOOFUS_WIRE_FUSED_INTERNAL_H
#define HADOOFUS_WIRE_FUSED_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_internal.h"

namespace hdfs_wire_fused {

using hdfs_wire::Pkt;
using hdfs_wire::Write;  // Write::crc and Write::slices are unused here: there is no CRC array

constexpr uint32_t kMaxGroups = 1024;  // workgroups of one launch

// Once per device, before the first launch there: the kernel's LDS (the table
// image, more than 64 KiB) is allowed.
hipError_t prepare_frame_fused();

// Writes wire[0, wire_len) of the write, chunk CRCs included: `groups`
// workgroups of 1024 (1 <= groups <= kMaxGroups), workgroup b taking packets
// b, b + groups, ...  tab: the compact tables (wire_fused_crc.h) of the
// write's polynomial in device memory; unused without csum.
hipError_t launch_frame_fused(const Write &w, const uint32_t *tab, uint32_t groups, hipStream_t stream);

}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_INTERNAL_H
