// Shared between md5crc_streams.cpp (host entry points) and
// md5crc_streams_kernels.hip.
#ifndef HADOOFUS_MD5CRC_STREAMS_INTERNAL_H
#define HADOOFUS_MD5CRC_STREAMS_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "md5_core.h"
#include "md5crc_streams_lookup.h"
#include "read_batch_layout.h"

namespace hdfs_md5crc_streams {

using hdfs_read_batch::Desc;
using hdfs_read_batch::kMaxEntries;
using hdfs_read_batch::kNoSlot;

static_assert(kTailRegions == hdfs_read_batch::kMaxTail, "a region per tail packet");

constexpr uint32_t kCheckWaves = 4;        // waves of a workgroup of the header check, a packet each a step
constexpr uint32_t kCheckMaxGroups = 2048;  // its workgroups at most
constexpr uint32_t kGatherThreads = 64;

// One entry as uploaded.
struct Entry {
  const uint8_t *stream;
  uint64_t len;
};

// The CRC regions of a regular entry, from the probe's descriptor: lengths only.
HDFS_HD Regions regions_of(const Desc &d, const uint8_t *stream, uint32_t entry) {
  Regions r;
  r.base = reinterpret_cast<uintptr_t>(stream);
  r.limit = d.consumed;
  r.stride = d.stride;
  r.hb0 = d.hb0;
  r.wpp = d.dlen0 / hdfs_read_batch::kChunk;
  r.nbody = d.nbody;
  r.ntail = d.ntail;
  const bool t0 = d.ntail > 0u, t1 = d.ntail > 1u, t2 = d.ntail > 2u;
  r.tail_off0 = t0 ? d.tail[0].stream_off + d.tail[0].hb : 0u;
  r.tail_off1 = t1 ? d.tail[1].stream_off + d.tail[1].hb : 0u;
  r.tail_off2 = t2 ? d.tail[2].stream_off + d.tail[2].hb : 0u;
  r.tail_words0 = t0 ? hdfs_read_batch::crc_count(d.tail[0].dlen) : 0u;
  r.tail_words1 = t1 ? hdfs_read_batch::crc_count(d.tail[1].dlen) : 0u;
  r.tail_words2 = t2 ? hdfs_read_batch::crc_count(d.tail[2].dlen) : 0u;
  r.nwords = count_words(r);
  r.nblk = uint32_t(hdfs_md5crc::md5_words_blocks(r.nwords));  // a stream is below 2^63 bytes
  r.entry = entry;
  return r;
}

// The device tables of one call, one allocation (n: the call's entries):
//   Entry    in[n]        uploaded: the entries' streams
//   uint32_t digest[4 n]  by slot: the MD5 state behind the last block
//   Regions  reg[n]       by slot: the entry's CRC regions
//   Desc     desc[n]      written by the probe: the regular entries, in batch
//                         order, slot s at desc[s]
//   uint32_t slot[n]      entry e's slot, or kNoSlot (irregular)
//   uint32_t status[n]    by slot: 0, or nonzero when the header check met a
//                         header that is not the predicted one
//   uint32_t pk0[n + 1]   by slot: packets of the regular entries ahead
//   uint32_t meta[2]      nreg, pk0[nreg]
// Everything from digest on comes back in one copy.
struct Tables {
  size_t in, digest, reg, desc, slot, status, pk0, meta, bytes;
  explicit Tables(size_t n) {
    in = 0;
    digest = in + n * sizeof(Entry);
    reg = digest + n * 16;
    desc = reg + n * sizeof(Regions);
    slot = desc + n * sizeof(Desc);
    status = slot + n * sizeof(uint32_t);
    pk0 = status + n * sizeof(uint32_t);
    meta = pk0 + (n + 1) * sizeof(uint32_t);
    bytes = meta + 2 * sizeof(uint32_t);
  }
};
static_assert(sizeof(Entry) % 16 == 0 && sizeof(Regions) % 16 == 0 && sizeof(Desc) % 8 == 0,
              "the digests are 16-byte aligned, the tables behind them 8-byte");

// A packet's CRC region to gather: bytes [src, src + bytes) to scratch + dst.
struct GatherRec {
  uint64_t src, dst;
  uint32_t bytes, reserved;
};

// The probe: one workgroup, thread e frames entry e < n (1 <= n <= kMaxEntries)
// and writes desc, reg, slot, status, pk0 and meta of the tables at `tables`.
hipError_t launch_probe_streams(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype,
                                hipStream_t stream);
// The header check, behind the probe on the same stream: `groups` workgroups of
// kCheckWaves waves, wave w of all taking packets w, w + waves, ... of the
// regular entries.
hipError_t launch_check_headers(void *tables, uint32_t n, uint32_t proto, uint32_t groups, hipStream_t stream);
// The digest, behind both: lane s digests reg[s] unless status[s] (may be NULL)
// is set, the MD5 state to digest + 4 s.  nreg is read from meta on the device
// (NULL: count entries).
hipError_t launch_digest_streams(const Regions *reg, const uint32_t *status, const uint32_t *meta, uint32_t count,
                                 uint32_t *digest, hipStream_t stream);
// The fallback's gather: record k's bytes to scratch, a workgroup each.
hipError_t launch_gather_regions(const GatherRec *recs, uint32_t nrec, uint8_t *scratch, hipStream_t stream);

}  // namespace hdfs_md5crc_streams

#endif  // HADOOFUS_MD5CRC_STREAMS_INTERNAL_H
