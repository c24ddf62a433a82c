// Shared between pread_batch.cpp (host entry points) and
// pread_batch_kernels.hip.
#ifndef HADOOFUS_PREAD_BATCH_INTERNAL_H
#define HADOOFUS_PREAD_BATCH_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pread_batch_layout.h"

namespace hdfs_pread_batch {

constexpr uint32_t kBatchMaxGroups = 1024;  // workgroups of the main launch

// The device tables of one call, one allocation (n: the call's entries):
//   Entry    in[n]        uploaded: the entries' streams, destinations and windows
//   Window   desc[n]      written by the probe: the regular entries, in batch
//                         order, slot s at desc[s]
//   uint32_t slot[n]      entry e's slot, or kNoSlot (irregular)
//   uint32_t status[n]    by slot: 0, or nonzero when the main launch met a
//                         header or a CRC that is not the expected one
//   uint32_t pk0[n + 1]   by slot: packets of the regular entries ahead;
//                         pk0[nreg]: all of them
//   uint32_t meta[2]      nreg, pk0[nreg]
// Everything from desc on comes back in one copy.
struct Tables {
  size_t in, desc, slot, status, pk0, meta, bytes;
  explicit Tables(size_t n) {
    in = 0;
    desc = in + n * sizeof(Entry);
    slot = desc + n * sizeof(Window);
    status = slot + n * sizeof(uint32_t);
    pk0 = status + n * sizeof(uint32_t);
    meta = pk0 + (n + 1) * sizeof(uint32_t);
    bytes = meta + 2 * sizeof(uint32_t);
  }
};
static_assert(sizeof(Entry) % 8 == 0 && sizeof(Window) % 8 == 0, "the tables behind are aligned");

// Once per device, before the first launch there: the main kernel's LDS (the
// table image, more than 64 KiB) is allowed.
hipError_t prepare_unframe_window_batch();

// The probe: one workgroup, thread e runs probe_window on entry e < n (1 <= n
// <= kMaxEntries) and writes desc, slot, status, pk0 and meta of the tables at
// `tables` (laid out by Tables(n)).
hipError_t launch_probe(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype, bool want_records,
                        uint64_t max_pkts, hipStream_t stream);

// The main launch, behind the probe on the same stream: `groups` workgroups of
// 1024 (1 <= groups <= kBatchMaxGroups), workgroup b taking global packets b,
// b + groups, ... of the regular entries' windows.  crc_tab: the compact tables
// (wire_fused_crc.h) of the batch's polynomial in device memory.
hipError_t launch_unframe_window_batch(void *tables, uint32_t n, uint32_t proto, const uint32_t *crc_tab,
                                       uint32_t groups, hipStream_t stream);

}  // namespace hdfs_pread_batch

#endif  // HADOOFUS_PREAD_BATCH_INTERNAL_H
