// Shared between relay_batch.cpp (host entry points) and
// relay_batch_kernels.hip.
#ifndef HADOOFUS_RELAY_BATCH_INTERNAL_H
#define HADOOFUS_RELAY_BATCH_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "read_batch_layout.h"
#include "relay_batch_lookup.h"

namespace hdfs_relay_batch {

using hdfs_read_batch::kMaxEntries;
using hdfs_read_batch::kMaxPackets;
using hdfs_read_batch::kNoSlot;

constexpr uint32_t kBatchMaxGroups = 1024;  // workgroups of the main launch

static_assert(kGrid == hdfs_read_batch::kChunk && kOutData == hdfs_read_batch::kMaxData, "one chunk, one packet size");

// One entry as uploaded.
struct Entry {
  const uint8_t *stream;
  uint64_t len;
  uint8_t *wire;
  uint64_t wire_cap;
  int64_t off, seq;  // the write's
  uint32_t finish, hb;  // hb: header bytes of an output packet
};

// What the probe leaves of an entry that takes the kernel: the read batch's
// descriptor of its input (dst unused), the same stream as a Geom, and the
// write's stream.
struct Desc {
  hdfs_read_batch::Desc in;
  Geom g;
  uint8_t *wire;
  uint64_t wire_len;
  int64_t off, seq;
  uint32_t npk;  // output packets, the empty last one of finish included
  uint32_t hb, finish, pad;
};

// The Geom of a regular entry's descriptor.
HDFS_HD Geom geom_of(const hdfs_read_batch::Desc &d) {
  Geom g;
  g.stride = d.stride;
  g.payload = d.delivered;
  g.cpp0 = d.dlen0 / kGrid;
  g.hb0 = d.hb0;
  g.K = d.nbody + 1u;
  const bool shorter = d.ntail >= 2u && d.tail[1].dlen != 0u;
  g.short_at = shorter ? d.tail[1].stream_off : 0u;
  g.short_dlen = shorter ? d.tail[1].dlen : 0u;
  g.short_hb = shorter ? d.tail[1].hb : 0u;
  // the stream's last packet, without an index computed at run time (the descriptor stays in registers)
  const uint32_t last_dlen = d.ntail == 3u ? d.tail[2].dlen : (d.ntail == 2u ? d.tail[1].dlen : d.tail[0].dlen);
  g.empty = last_dlen == 0u ? 1u : 0u;
  return g;
}

// The device tables of one call, one allocation (n: the call's entries), as
// read_batch_internal.h's:
//   Entry    in[n]        uploaded
//   Desc     desc[n]      written by the probe: the entries that take the
//                         kernel, in batch order, slot s at desc[s]
//   uint32_t slot[n]      entry e's slot, or kNoSlot
//   uint32_t status[n]    by slot: 0, or nonzero when the main launch met a
//                         header or a CRC that is not the expected one
//   uint32_t pk0[n + 1]   by slot: OUTPUT packets of the slots ahead;
//                         pk0[nreg]: all of them
//   uint32_t meta[2]      nreg, pk0[nreg]
// Everything from desc on comes back in one copy.
struct Tables {
  size_t in, desc, slot, status, pk0, meta, bytes;
  explicit Tables(size_t n) {
    in = 0;
    desc = in + n * sizeof(Entry);
    slot = desc + n * sizeof(Desc);
    status = slot + n * sizeof(uint32_t);
    pk0 = status + n * sizeof(uint32_t);
    meta = pk0 + (n + 1) * sizeof(uint32_t);
    bytes = meta + 2 * sizeof(uint32_t);
  }
};
static_assert(sizeof(Entry) % 8 == 0 && sizeof(Desc) % 8 == 0, "the tables behind are aligned");

// Once per device, before the first launch there: the main kernel's LDS (the
// table image, more than 64 KiB) is allowed.
hipError_t prepare_relay_fused_batch();

// The probe: one workgroup, thread e frames entry e < n (1 <= n <=
// kMaxEntries), decides whether it takes the kernel and writes desc, slot,
// status, pk0 and meta of the tables at `tables` (laid out by Tables(n)).
hipError_t launch_probe(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype, hipStream_t stream);

// The main launch, behind the probe on the same stream: `groups` workgroups of
// 1024 (1 <= groups <= kBatchMaxGroups), workgroup b taking global output
// packets b, b + groups, ... of the entries that have a slot.  crc_tab: the
// compact tables (wire_fused_crc.h) of the batch's polynomial in device memory.
hipError_t launch_relay_fused_batch(void *tables, uint32_t n, uint32_t proto, const uint32_t *crc_tab, uint32_t groups,
                                    hipStream_t stream);

}  // namespace hdfs_relay_batch

#endif  // HADOOFUS_RELAY_BATCH_INTERNAL_H
