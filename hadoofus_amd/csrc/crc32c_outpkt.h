// Write path: packet sizing and header buffers of outgoing data packets
// (_send_packet / _compose_data_packet_header).  One definition, shared by
// hdfs_crc32c_compose_packets (crc32c_packets.cpp) and the gather-write
// companion library (writev.cpp): both write byte-identical header buffers.
// Host code, except the byte writers marked HDFS_OUTPKT_HD: the wire-stream
// companion's kernel (wire_kernels.hip) writes a packet's header with them.
#ifndef HADOOFUS_CRC32C_OUTPKT_H
#define HADOOFUS_CRC32C_OUTPKT_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hadoofus_crc32c.h"

#if defined(__HIPCC__)
#define HDFS_OUTPKT_HD __host__ __device__
#else
#define HDFS_OUTPKT_HD
#endif

namespace hdfs_crc32c {
namespace outpkt {

constexpr int64_t kPacketSize = 64 * 1024;  // PACKET_SIZE, src/datanode.c:38
constexpr uint32_t kWriteChunk = 512;       // CHUNK_SIZE, src/datanode.c:37

struct OutPlan {
  int64_t offset;
  int64_t seqno;
  uint64_t data_off;
  int32_t dlen;
  bool last;
};

// Packet sizing of one write: src/datanode.c:2590 (min(remains_tot,
// PACKET_SIZE)) and :2592-2609 (an unaligned offset first completes its chunk).
inline void plan_out_packets(uint64_t len, int64_t off, int64_t seq, bool finish, std::vector<OutPlan> &v) {
  uint64_t pos = 0;
  while (pos < len) {
    int64_t n = int64_t(std::min<uint64_t>(len - pos, uint64_t(kPacketSize)));
    if (off % kWriteChunk) n = std::min<int64_t>(n, kWriteChunk - off % kWriteChunk);
    v.push_back(OutPlan{off, seq, pos, int32_t(n), false});
    off += n;
    pos += uint64_t(n);
    seq++;
  }
  // hdfs_datanode_finish_block: an empty packet, lastPacketInBlock = (remains_pkt == 0)
  if (finish) v.push_back(OutPlan{off, seq, pos, 0, true});
}

HDFS_OUTPKT_HD inline uint8_t *put_be(uint8_t *p, uint64_t v, int n) {
  for (int i = n - 1; i >= 0; i--) *p++ = uint8_t(v >> (8 * i));
  return p;
}
HDFS_OUTPKT_HD inline uint8_t *put_le(uint8_t *p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) *p++ = uint8_t(v >> (8 * i));
  return p;
}

// protobuf-c packing of PacketHeaderProto as the reference fills it
// (src/datanode.c:2795-2806): required fields in number order, sfixed64 /
// sfixed32 little-endian, the bool as a one-byte varint, syncBlock unset.
constexpr uint32_t kHdrProtoBytes = 25;
HDFS_OUTPKT_HD inline uint8_t *put_header_proto(uint8_t *p, int64_t off, int64_t seq, bool last, int32_t dlen) {
  *p++ = 0x09;  // field 1, wire type 1 (64-bit)
  p = put_le(p, uint64_t(off), 8);
  *p++ = 0x11;  // field 2, wire type 1
  p = put_le(p, uint64_t(seq), 8);
  *p++ = 0x18;  // field 3, wire type 0 (varint)
  *p++ = last ? 1 : 0;
  *p++ = 0x25;  // field 4, wire type 5 (32-bit)
  return put_le(p, uint32_t(dlen), 4);
}

HDFS_OUTPKT_HD inline uint32_t out_header_bytes(int proto) { return proto == HDFS_CRC32C_PROTO_V1 ? 25u : 4u + 2u + kHdrProtoBytes; }

// One packet's header bytes alone -- plen, then hlen + PacketHeaderProto (v2)
// or the v1 header -- as write_out_packets writes them ahead of the packet's
// ncrc chunk CRCs: out_header_bytes(proto) bytes at p.
HDFS_OUTPKT_HD inline uint8_t *put_out_header(uint8_t *p, int proto, int64_t off, int64_t seq, bool last,
                                              int32_t dlen, uint64_t ncrc) {
  p = put_be(p, uint64_t(uint32_t(int32_t(dlen + 4 * ncrc + 4))), 4);  // plen (src/datanode.c:2792)
  if (proto == HDFS_CRC32C_PROTO_V2) {
    p = put_be(p, kHdrProtoBytes, 2);  // hlen (s16)
    return put_header_proto(p, off, seq, last, dlen);
  }
  p = put_be(p, uint64_t(off), 8);  // src/datanode.c:2808-2812
  p = put_be(p, uint64_t(seq), 8);
  *p++ = last ? 1 : 0;
  return put_be(p, uint32_t(dlen), 4);
}

// Header bytes the plan's packets need (csum: 4 CRC bytes per chunk).
inline uint64_t out_plan_bytes(const std::vector<OutPlan> &plan, int proto, bool csum) {
  const uint32_t hb = out_header_bytes(proto);
  uint64_t need = 0;
  for (const OutPlan &k : plan)
    need += hb + (csum ? 4ull * ((uint64_t(k.dlen) + kWriteChunk - 1) / kWriteChunk) : 0ull);
  return need;
}

// Bytes of the write's first packet when it is the single short chunk that
// completes an unaligned block offset's chunk (0: the write starts on the
// chunk grid, or is empty).
inline uint64_t out_head_bytes(const std::vector<OutPlan> &plan, uint64_t len, int64_t offset_in_block) {
  return (len && offset_in_block % kWriteChunk) ? uint64_t(plan[0].dlen) : 0;
}

// The header buffers and packet records of a planned write.  The chunk CRCs
// are in wire (BE) byte order already: head[0] that of the short first chunk
// (n0 > 0), body[] those of the 512-B grid that starts n0 bytes into the
// write.  out has out_plan_bytes(), pkts plan.size() entries.
inline void write_out_packets(const std::vector<OutPlan> &plan, int proto, bool csum, uint64_t n0,
                              const uint32_t *head, const uint32_t *body, uint8_t *out,
                              hdfs_crc32c_out_packet *pkts) {
  uint64_t pos = 0;
  for (size_t i = 0; i < plan.size(); i++) {
    const OutPlan &k = plan[i];
    const uint64_t ncrc = csum ? (uint64_t(k.dlen) + kWriteChunk - 1) / kWriteChunk : 0;
    uint8_t *p = out + pos;
    p = put_be(p, uint64_t(uint32_t(int32_t(k.dlen + 4 * ncrc + 4))), 4);  // plen (src/datanode.c:2792)
    if (proto == HDFS_CRC32C_PROTO_V2) {
      p = put_be(p, kHdrProtoBytes, 2);  // hlen (s16)
      p = put_header_proto(p, k.offset, k.seqno, k.last, k.dlen);
    } else {  // src/datanode.c:2808-2812
      p = put_be(p, uint64_t(k.offset), 8);
      p = put_be(p, uint64_t(k.seqno), 8);
      *p++ = k.last ? 1 : 0;
      p = put_be(p, uint32_t(k.dlen), 4);
    }
    if (ncrc) {  // CRCs are already in wire (BE) byte order
      const uint32_t *src = (n0 && i == 0) ? head : body + (k.data_off - n0) / kWriteChunk;
      std::memcpy(p, src, size_t(ncrc) * 4);
      p += ncrc * 4;
    }
    hdfs_crc32c_out_packet &o = pkts[i];
    std::memset(&o, 0, sizeof(o));
    o.hdr_off = pos;
    o.data_off = k.data_off;
    o.offset_in_block = k.offset;
    o.seqno = k.seqno;
    o.data_len = k.dlen;
    o.hdr_len = uint32_t(p - (out + pos));
    o.crc_len = uint32_t(ncrc * 4);
    o.last = k.last ? 1 : 0;
    pos += o.hdr_len;
  }
}

}  // namespace outpkt
}  // namespace hdfs_crc32c

#endif  // HADOOFUS_CRC32C_OUTPKT_H
