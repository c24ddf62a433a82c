// Shared between md5crc.cpp (host entry points) and md5crc_kernels.hip.
#ifndef HADOOFUS_MD5CRC_INTERNAL_H
#define HADOOFUS_MD5CRC_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdfs_md5crc {

// One segment as the kernel sees it: its chunk-CRC array and how to read it.
struct SegTab {
  const uint32_t *crcs;  // device u32[nchunks], 4-byte aligned (NULL when nchunks == 0)
  uint32_t nchunks;
  uint32_t be;           // 1: the words are already in wire order
};
static_assert(sizeof(SegTab) == 16, "SegTab layout");

// digests[4 * i .. 4 * i + 3] = MD5 of segment i's CRCs in wire order; one
// lane per segment, one wave per workgroup.  digests: 16-byte aligned device
// memory, 16 * nseg bytes.
hipError_t launch_block_digests(const SegTab *tab, uint32_t nseg, uint32_t *digests, hipStream_t stream);

}  // namespace hdfs_md5crc

#endif  // HADOOFUS_MD5CRC_INTERNAL_H
