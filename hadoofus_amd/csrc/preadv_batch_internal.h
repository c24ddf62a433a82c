// Shared between preadv_batch.cpp (host entry points) and
// preadv_batch_kernels.hip.
#ifndef HADOOFUS_PREADV_BATCH_INTERNAL_H
#define HADOOFUS_PREADV_BATCH_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pread_batch_internal.h"
#include "pread_batch_layout.h"
#include "wirev_fused_internal.h"

namespace hdfs_preadv_batch {

using hdfs_pread_batch::Desc;
using hdfs_pread_batch::Entry;  // Entry::dst is unused here (NULL); Entry::dst_cap is the fragments' total, cap
using hdfs_pread_batch::kMaxEntries;
using hdfs_pread_batch::kNoSlot;
using hdfs_pread_batch::Window;  // Desc::dst is unused here: Desc::entry leads from a slot to its fragments
using hdfs_wirev_fused::Frag;

constexpr uint32_t kBatchMaxGroups = 1024;  // workgroups of the main launch

// The device tables of one call, one allocation, in an order that keeps Frag
// 16-byte aligned (n: the call's entries, nfe: the rows of the fragment table,
// every entry's sentinel included):
//   Frag     ft[nfe]      entry after entry, each entry's non-empty fragments
//                         with `at` rising strictly from 0 inside the entry,
//                         then its own sentinel {NULL, cap}: the layout of
//                         wirev_fused_batch_internal.h, its bases destinations
//   uint32_t fr0[n + 1]   fr0[e]: index of ENTRY e's first Frag (by entry, not
//                         by slot: the probe deals the slots on the device,
//                         the host lays the fragments); fr0[n] == nfe
//   then the pread batch's tables (pread_batch_internal.h, Tables(n)) from
//   `base` on: in[n], desc[n], slot[n], status[n], pk0[n + 1], meta[2].
// Everything up to the end of in[] goes up in one copy; everything from desc
// on comes back in one copy.
struct Tables {
  hdfs_pread_batch::Tables p;
  size_t ft, fr0, base, up, bytes;
  Tables(size_t n, size_t nfe) : p(n) {
    ft = 0;
    fr0 = nfe * sizeof(Frag);
    base = (fr0 + (n + 1) * sizeof(uint32_t) + 15u) / 16u * 16u;
    up = base + p.desc;
    bytes = base + p.bytes;
  }
};

// Once per device, before the first launch there: the main kernel's LDS (the
// table image, more than 64 KiB) is allowed.
hipError_t prepare_unframe_scatter_batch();

// The probe: one workgroup, thread e runs probe_window on entry e < n (1 <= n
// <= kMaxEntries) with dst_cap = the entry's cap and writes desc, slot, status,
// pk0 and meta of the tables at `tables` (laid out by Tables(n, nfe)).
hipError_t launch_probe(void *tables, uint32_t n, uint32_t nfe, int proto, uint32_t chunk_size, int ctype,
                        bool want_records, uint64_t max_pkts, hipStream_t stream);

// The main launch, behind the probe on the same stream: `groups` workgroups of
// 1024 (1 <= groups <= kBatchMaxGroups), workgroup b taking global packets b,
// b + groups, ... of the regular entries' windows.  crc_tab: the compact tables
// (wire_fused_crc.h) of the batch's polynomial in device memory.
hipError_t launch_unframe_scatter_batch(void *tables, uint32_t n, uint32_t nfe, uint32_t proto,
                                        const uint32_t *crc_tab, uint32_t groups, hipStream_t stream);

}  // namespace hdfs_preadv_batch

#endif  // HADOOFUS_PREADV_BATCH_INTERNAL_H
