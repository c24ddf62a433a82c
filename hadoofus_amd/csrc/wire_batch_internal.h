// Shared between wire_batch.cpp (host entry points) and wire_batch_kernels.hip.
#ifndef HADOOFUS_WIRE_BATCH_INTERNAL_H
#define HADOOFUS_WIRE_BATCH_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_internal.h"

namespace hdfs_wire {

// Workgroups per packet of the batch kernel: frame_packets_kernel's measured
// choice (kSlices, wire_layout.h), here a compile-time constant.
constexpr uint32_t kBatchSlices = 4;

// The device tables of one batch, one allocation, one upload:
//   Write    tab[nw]      the writes that have packets, in batch order, every
//                         pointer set (crc: the write's slice of the CRC array)
//   uint32_t pk0[nw + 1]  pk0[k]: packets of the writes ahead of write k;
//                         pk0[nw]: all of them
// The host drops writes without packets, so pk0 rises strictly and the search
// for the k with pk0[k] <= g < pk0[k + 1] has one answer.
inline size_t batch_table_bytes(size_t nw) { return nw * sizeof(Write) + (nw + 1) * sizeof(uint32_t); }
static_assert(sizeof(Write) % sizeof(uint64_t) == 0, "pk0 behind the table is aligned");

// Frames every packet of the nw writes of the tables at tab: total_pk *
// kBatchSlices workgroups of 256.  1 <= nw, pk0[nw] == total_pk >= nw.
hipError_t launch_frame_batch(const void *tab, uint32_t nw, uint32_t total_pk, hipStream_t stream);

}  // namespace hdfs_wire

#endif  // HADOOFUS_WIRE_BATCH_INTERNAL_H
