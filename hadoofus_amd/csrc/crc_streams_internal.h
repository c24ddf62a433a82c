// Shared between crc_streams.cpp (host entry points) and
// crc_streams_kernels.hip.
#ifndef HADOOFUS_CRC_STREAMS_INTERNAL_H
#define HADOOFUS_CRC_STREAMS_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "crc32c_tables.h"
#include "crc_streams_lookup.h"
#include "read_batch_layout.h"

namespace hdfs_crc_streams {

using hdfs_read_batch::Desc;
using hdfs_read_batch::kMaxEntries;
using hdfs_read_batch::kNoSlot;

static_assert(kTailPackets == hdfs_read_batch::kMaxTail, "a length per tail packet");

constexpr uint32_t kFoldWaves = 4;         // waves of a workgroup of the fold, a packet each a step
constexpr uint32_t kFoldMaxGroups = 2048;  // its workgroups at most
// A regular packet is at least 25 header bytes, one CRC and 512 data bytes on
// the wire, so a stream of len bytes has at most len / kMinPacketWire + 3
// packets: what the per-packet table is sized by before the probe has run.
constexpr uint32_t kMinPacketWire = 25 + 4 + 512;
// ... up to this many packets a call (128 MiB of table).  The entries whose
// packets lie past it are flagged by the fold and take the fallback.
constexpr uint32_t kPacketBudget = 1u << 25;

// One entry as uploaded.
struct Entry {
  const uint8_t *stream;
  uint64_t len;
};

// The data lengths of a regular entry, from the probe's descriptor.
HDFS_HD Shape shape_of(const Desc &d) {
  Shape s;
  s.nbody = d.nbody;
  s.ntail = d.ntail;
  s.dlen0 = d.dlen0;
  s.tail0 = d.ntail > 0u ? d.tail[0].dlen : 0u;
  s.tail1 = d.ntail > 1u ? d.tail[1].dlen : 0u;
  s.tail2 = d.ntail > 2u ? d.tail[2].dlen : 0u;
  return s;
}

// The multiplier table (crc_streams_lookup.h: kMult*) of a polynomial and a
// chunk size, on the host, with crc32c_tables.h's operator.
inline void make_multipliers(uint32_t *mult, uint32_t poly, uint32_t chunk_size) {
  using hdfs_crc32c::Gf2;
  const Gf2 zc = hdfs_crc32c::zeros_op(chunk_size, poly);
  mult[kMultLane + kLanes - 1u] = kOne;
  for (uint32_t l = kLanes - 1u; l > 0u; l--) mult[kMultLane + l - 1u] = zc.apply(mult[kMultLane + l]);
  mult[kMultStep] = zc.apply(mult[kMultLane]);
  mult[kMultPoly] = poly;
  mult[kMultChunk] = chunk_size;
  mult[kMultChunk + 1u] = 0u;
  Gf2 p = Gf2::one_zero_byte(poly);
  for (uint32_t b = 0; b < 64u; b++) {
    mult[kMultPow2 + b] = p.apply(kOne);
    p = p.compose(p);
  }
}

// A packet as hdfs_crc32c_parse_packets framed it (the described-packet path).
struct PktRec {
  uint64_t addr;   // its CRC region: 4 ncrc bytes of device memory
  uint64_t after;  // payload bytes of its entry behind it
  uint32_t ncrc;
  uint32_t dlen;
};
// A described entry: packets [p0, p0 + npk) of the PktRec table.
struct Span {
  uint32_t p0, npk;
};

// The device tables of one call, one allocation (n: the call's entries):
//   Entry    in[n]        uploaded: the entries' streams
//   uint32_t mult[132]    uploaded with them: the multipliers (crc_streams_lookup.h)
//   Desc     desc[n]      written by the probe: the regular entries, in batch
//                         order, slot s at desc[s]
//   uint32_t crc[n]       by slot: the entry's CRC
//   uint32_t slot[n]      entry e's slot, or kNoSlot (irregular)
//   uint32_t status[n]    by slot: 0, or nonzero when the fold met a header
//                         that is not the predicted one or ran out of table
//   uint32_t pk0[n + 1]   by slot: packets of the regular entries ahead
//   uint32_t meta[2]      nreg, pk0[nreg]
// in and mult go up in one copy; everything from desc on comes back in one.
struct Tables {
  size_t in, mult, desc, crc, slot, status, pk0, meta, bytes;
  explicit Tables(size_t n) {
    in = 0;
    mult = in + n * sizeof(Entry);
    desc = mult + kMultWords * sizeof(uint32_t);
    crc = desc + n * sizeof(Desc);
    slot = crc + n * sizeof(uint32_t);
    status = slot + n * sizeof(uint32_t);
    pk0 = status + n * sizeof(uint32_t);
    meta = pk0 + (n + 1) * sizeof(uint32_t);
    bytes = meta + 2 * sizeof(uint32_t);
  }
};
static_assert(sizeof(Entry) % 16 == 0 && (kMultWords * 4) % 16 == 0 && sizeof(Desc) % 8 == 0,
              "the descriptors are 8-byte aligned");
static_assert(sizeof(PktRec) == 24 && sizeof(Span) == 8, "the described path's tables");

// The probe: one workgroup, thread e frames entry e < n (1 <= n <= kMaxEntries)
// and writes desc, slot, status, pk0 and meta of the tables at `tables`.
hipError_t launch_probe_streams(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype,
                                hipStream_t stream);
// Check and fold, behind the probe on the same stream: `groups` workgroups of
// kFoldWaves waves, wave w of all taking packets w, w + waves, ... of the
// regular entries; packet g's CRC goes to cp[g], g < cap.
hipError_t launch_fold_streams(void *tables, uint32_t n, uint32_t proto, uint32_t groups, uint32_t *cp, uint32_t cap,
                               hipStream_t stream);
// The reduce, behind both: wave s reduces slot s unless its status is set; the
// entry's CRC to the tables' crc[s].
hipError_t launch_reduce_streams(void *tables, uint32_t n, const uint32_t *cp, uint32_t cap, hipStream_t stream);
// The same two kernels over described packets: recs[0 .. nrec) folded into
// cp[0 .. nrec), spans[0 .. nspan) reduced into out[0 .. nspan).  mult: a
// multiplier table in device memory.
hipError_t launch_fold_described(const PktRec *recs, uint32_t nrec, const uint32_t *mult, uint32_t groups, uint32_t *cp,
                                 hipStream_t stream);
hipError_t launch_reduce_described(const Span *spans, uint32_t nspan, const PktRec *recs, uint32_t nrec,
                                   const uint32_t *mult, const uint32_t *cp, uint32_t *out, hipStream_t stream);

}  // namespace hdfs_crc_streams

#endif  // HADOOFUS_CRC_STREAMS_INTERNAL_H
