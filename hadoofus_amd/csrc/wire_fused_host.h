// Host side shared by the four fused wire-stream libraries (wire_fused.cpp,
// wire_fused_batch.cpp, wirev_fused.cpp, wirev_fused_batch.cpp): what each
// keeps on the engine's device once it has been used there, and how a call
// picks its table half and its grid.  One definition, included by all four; no
// kernel file includes it.
#ifndef HADOOFUS_WIRE_FUSED_HOST_H
#define HADOOFUS_WIRE_FUSED_HOST_H

#include <vector>

#include "companion_support.h"
#include "wire_fused_tables.h"

namespace hdfs_wire_fused {

// Prepare: the library's prepare_* (its kernel's LDS is allowed).  MaxGroups:
// the most workgroups its launch takes.
template <hipError_t (*Prepare)(), uint32_t MaxGroups>
struct DeviceState {
  hdfs_companion::DeviceBuffer crc_tab;  // the compact tables of both polynomials, CRC32C first
  uint32_t groups = 0;                   // the workgroups of one launch: one per CU, 1 to MaxGroups
  bool ready = false;

  // Once on device `dev` (the current one): the tables uploaded, the kernel
  // prepared, the CUs counted.
  int setup(int dev) {
    using namespace hdfs_companion;
    if (ready) return HDFS_CRC32C_OK;
    std::vector<uint32_t> host(2 * crc::kCompactWords);
    crc::make_compact(hdfs_crc32c::kPoly, host.data());
    crc::make_compact(hdfs_crc32c::kPolyZlib, host.data() + crc::kCompactWords);
    const int rc = crc_tab.reserve(host.size() * sizeof(uint32_t), 0);
    if (rc) return rc;
    int cus = 0;
    hipError_t e = hipMemcpy(crc_tab.p, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e == hipSuccess) e = Prepare();
    if (e != hipSuccess) return fail(HDFS_CRC32C_EHIP, "tables: %s", hipGetErrorString(e));
    groups = cus < 1 ? 1u : (uint32_t(cus) > MaxGroups ? MaxGroups : uint32_t(cus));
    ready = true;
    return HDFS_CRC32C_OK;
  }
  void release() {
    crc_tab.release();
    ready = false;
  }

  // The timing calls' flags: the workgroups asked for in the bits above the
  // low eight (0: the product's grid), nothing else.
  static int flags_ok(unsigned flags) {
    if ((flags & 0xFFu) || (flags >> 8) > MaxGroups)
      return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "1 to %u workgroups", MaxGroups);
    return HDFS_CRC32C_OK;
  }
  // The compact tables of ctype's polynomial.
  const uint32_t *tables(int ctype) const {
    return crc_tab.as<uint32_t>() + (ctype == HDFS_CRC32C_CSUM_CRC32 ? crc::kCompactWords : 0u);
  }
  // The product's grid: a workgroup per CU, and none without a packet.
  uint32_t grid(unsigned flags, uint32_t packets) const {
    const unsigned want = flags >> 8;
    return want ? want : (packets < groups ? packets : groups);
  }
};

}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_HOST_H
