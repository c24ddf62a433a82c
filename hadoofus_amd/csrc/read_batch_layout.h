// The arithmetic of libhadoofus_read_batch.so's probe, written once for host
// and device: probe_kernel (read_batch_kernels.hip) runs it with one thread per
// entry on the streams in device memory, read_batch.cpp synthesises the packet
// records from its result, and tests/consumer/read_batch_selftest.cpp runs the
// same functions on host-built streams against a brute-force frame_step walk.
// No HIP runtime call is made here.
//
// A datanode's read stream is K packets of one size whose data is a whole
// number of 512-B chunks, at most one shorter data packet and at most one
// empty lastPacketInBlock packet.  Packet 0 is framed with frame::frame_step
// (crc32c_frame.h, the definition the main library walks with); its wire size
// is the stride, and K follows from the stream's length: the largest of
// len / stride, len / stride - 1, len / stride - 2 at which packet K - 1,
// framed at (K - 1) * stride, is again a complete clean packet of packet 0's
// sizes (what follows the run -- a shorter packet, an empty one, a cut packet
// -- is less than three strides).  From packet K - 1 on the stream is framed
// with frame_step, at most kMaxTail packets: these are the entry's tail and
// are taken as framed.  Packets 0 .. K - 2 are the body: predicted from
// packet 0 (offsetInBlock + dlen0 and seqno + 1 per packet, the same flags,
// the same header length), never framed here.  unframe_fused_batch_kernel
// compares every header, body and tail, with the bytes the prediction
// composes, so a stream whose body is not the prediction is flagged there and
// goes to hdfs_crc32c_read_packets; when every header matches, the chain of
// strides is the stream's own and this layout is what the main library's walk
// finds.
//
// An entry is REGULAR when chunk_size is 512, packet 0 is complete and clean
// with a header of the canonical length (25 B v1; 31 B v2, 33 B with
// syncBlock), dlen0 is a multiple of 512 in [512, 65536], the tail is as
// above and ends at the stream's end, at an incomplete packet or with the
// empty last packet, the payload fits dst_cap and (records wanted) the
// packets fit max_pkts.  Everything else is irregular: no packets, no access
// by the main launch.  For a regular entry
//   nbody * stride + (tail bytes) == consumed <= len,  delivered <= dst_cap,
// every packet's header, CRC and data regions lie in [0, consumed) and its
// destination bytes in [0, delivered): the kernel's accesses follow from the
// descriptor alone.
#ifndef HADOOFUS_READ_BATCH_LAYOUT_H
#define HADOOFUS_READ_BATCH_LAYOUT_H

#include <stdint.h>

#include "crc32c_frame.h"

namespace hdfs_read_batch {

constexpr uint32_t kChunk = 512;
constexpr uint32_t kMaxData = 65536;                // most data bytes of a packet the kernel takes (16 rounds)
constexpr uint32_t kMaxTail = 3;                    // packet K - 1, a shorter one, the empty last one
constexpr uint32_t kMaxEntries = 1024;              // one probe thread per entry, one workgroup
constexpr uint32_t kMaxPackets = 0x7FFFFFFFu / 4u;  // of one launch, as the fused batch write libraries
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;

// One entry as uploaded.
struct Entry {
  const uint8_t *stream;
  uint64_t len;
  uint8_t *dst;
  uint64_t dst_cap;
};

// A packet as framed (tail) or predicted (body).
struct PacketAt {
  uint64_t stream_off, dst_off;
  int64_t off, seq;
  uint32_t dlen, hb;    // data bytes; header bytes ahead of the CRCs
  uint32_t last, sync;  // the record's flags (0 / 1)
};

// What the probe leaves of a regular entry.
struct Desc {
  const uint8_t *stream;
  uint8_t *dst;
  uint64_t stride;               // wire bytes of a body packet
  uint64_t consumed, delivered;  // hdfs_crc32c_read_packets' of a clean stream
  int64_t off0, seq0;
  uint32_t dlen0, hb0, last0, sync0;
  uint32_t nbody, ntail, npk;  // npk = nbody + ntail
  uint32_t entry;              // index in the batch
  PacketAt tail[kMaxTail];
};

HDFS_HD uint32_t canonical_header(int proto) { return proto == HDFS_CRC32C_PROTO_V1 ? 25u : 31u; }
// v2 with syncBlock: two more bytes.
HDFS_HD bool header_len_ok(int proto, uint32_t hb) {
  const uint32_t base = canonical_header(proto);
  return hb == base || (proto == HDFS_CRC32C_PROTO_V2 && hb == base + 2u);
}
HDFS_HD bool has_sync(int proto, uint32_t hb) { return hb != canonical_header(proto); }
HDFS_HD uint32_t crc_count(uint32_t dlen) { return (dlen + kChunk - 1u) / kChunk; }

HDFS_HD PacketAt framed(const hdfs_crc32c_packet &k, uint64_t dst_off) {
  return PacketAt{k.stream_off, dst_off, k.offset_in_block, k.seqno, uint32_t(k.data_len), k.header_len,
                  k.last ? 1u : 0u, k.sync ? 1u : 0u};
}

// Packet i < d.npk of a regular entry.
HDFS_HD PacketAt packet_of(const Desc &d, uint32_t i) {
  if (i >= d.nbody) return d.tail[i - d.nbody];
  return PacketAt{uint64_t(i) * d.stride, uint64_t(i) * d.dlen0, d.off0 + int64_t(uint64_t(i) * d.dlen0),
                  d.seq0 + int64_t(i), d.dlen0, d.hb0, d.last0, d.sync0};
}

// The record hdfs_crc32c_read_packets gives a clean packet.
HDFS_HD hdfs_crc32c_packet record_of(const PacketAt &p) {
  hdfs_crc32c_packet k = hdfs_crc32c_packet{};
  k.stream_off = p.stream_off;
  k.offset_in_block = p.off;
  k.seqno = p.seq;
  k.data_len = int32_t(p.dlen);
  k.crc_len = int32_t(4u * crc_count(p.dlen));
  k.header_len = p.hb;
  k.first_bad = -1;
  k.last = uint8_t(p.last);
  k.sync = uint8_t(p.sync);
  return k;
}

// at(pos): the stream's bytes from pos on (frame_step reads the packet's header
// there and nothing else).  Fills d but stream, dst and entry.  -> regular.
template <class At>
HDFS_HD bool probe_entry(At at, uint64_t len, uint64_t dst_cap, int proto, uint32_t chunk_size, int ctype,
                         bool want_records, uint64_t max_pkts, Desc &d) {
  using namespace hdfs_crc32c::frame;
  d.stride = d.consumed = d.delivered = 0;
  d.off0 = d.seq0 = 0;
  d.dlen0 = d.hb0 = d.last0 = d.sync0 = d.nbody = d.ntail = d.npk = 0;
  if (chunk_size != kChunk || !len) return false;
  hdfs_crc32c_packet k0, k;
  uint64_t total = 0;
  if (frame_step(at(uint64_t(0)), len, 0, proto, chunk_size, ctype, k0, total) != kStepNext) return false;
  if (!header_len_ok(proto, k0.header_len)) return false;
  const uint32_t dlen0 = uint32_t(k0.data_len);
  if (dlen0 < kChunk || dlen0 > kMaxData || dlen0 % kChunk) return false;
  const uint64_t stride = total, kc = len / stride;  // kc >= 1: packet 0 is complete
  uint64_t K = 0;
  for (uint64_t c = 0; c < 3u && c < kc; c++) {
    const uint64_t cand = kc - c, pos = (cand - 1u) * stride;
    k = k0;
    if (cand > 1u && (frame_step(at(pos), len - pos, pos, proto, chunk_size, ctype, k, total) != kStepNext ||
                      k.header_len != k0.header_len || uint32_t(k.data_len) != dlen0))
      continue;
    K = cand;
    break;
  }
  if (!K) return false;
  if (K - 1u > kMaxPackets) return false;
  uint64_t pos = K * stride, payload = K * dlen0;
  d.tail[0] = framed(k, (K - 1u) * dlen0);
  uint32_t nt = 1;
  // at most one shorter data packet, then at most the empty last packet
  for (uint32_t s = 1; s < kMaxTail && pos < len; s++) {
    const int r = frame_step(at(pos), len - pos, pos, proto, chunk_size, ctype, k, total);
    if (r == kStepMore) break;  // incomplete: the walk ends ahead of it
    if (k.error || !header_len_ok(proto, k.header_len)) return false;
    if (r == kStepStop) {  // the empty last packet ends the walk
      if (s == 1)
        d.tail[1] = framed(k, payload);
      else
        d.tail[2] = framed(k, payload);
      nt++;
      pos += total;
      break;
    }
    if (s != 1 || uint32_t(k.data_len) >= dlen0) return false;  // a second short packet, or a size break
    d.tail[1] = framed(k, payload);
    nt++;
    pos += total;
    payload += uint32_t(k.data_len);
  }
  const uint64_t npk = K - 1u + nt;
  if (payload > dst_cap || npk > kMaxPackets || (want_records && npk > max_pkts)) return false;
  d.stride = stride;
  d.consumed = pos;
  d.delivered = payload;
  d.off0 = k0.offset_in_block;
  d.seq0 = k0.seqno;
  d.dlen0 = dlen0;
  d.hb0 = k0.header_len;
  d.last0 = k0.last ? 1u : 0u;
  d.sync0 = k0.sync ? 1u : 0u;
  d.nbody = uint32_t(K - 1u);
  d.ntail = nt;
  d.npk = uint32_t(npk);
  return true;
}

// The packet-count prefix over the regular entries: npk[e] is entry e's
// packets (0: irregular).  slot[e]: its place among the regular ones, or
// kNoSlot; pk0[0 .. nreg] rises strictly from 0 (wire_fused_batch_lookup.h's
// array).  An entry that would take the launch past kMaxPackets is left out.
// -> nreg.
HDFS_HD uint32_t prefix_regular(const uint32_t *npk, uint32_t n, uint32_t *slot, uint32_t *pk0) {
  uint32_t nreg = 0, total = 0;
  for (uint32_t e = 0; e < n; e++) {
    const uint32_t c = npk[e] <= kMaxPackets - total ? npk[e] : 0u;
    slot[e] = c ? nreg : kNoSlot;
    if (!c) continue;
    pk0[nreg++] = total;
    total += c;
  }
  pk0[nreg] = total;
  return nreg;
}

}  // namespace hdfs_read_batch

#endif  // HADOOFUS_READ_BATCH_LAYOUT_H
