// Shared between wire.cpp (host entry points) and wire_kernels.hip.
#ifndef HADOOFUS_WIRE_INTERNAL_H
#define HADOOFUS_WIRE_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdfs_wire {

constexpr uint32_t kChunk = 512;        // outpkt::kWriteChunk
constexpr uint32_t kPacket = 64 * 1024;  // outpkt::kPacketSize
constexpr uint32_t kMaxSlices = 16;

// One write, as the frame kernel sees it.  Header lengths are constant per
// protocol and only the first and the last data packet can be short, so
// every packet's place follows from its index (packet_at).
struct Write {
  const uint8_t *data;  // len bytes
  const uint32_t *crc;  // u32[chunks of the write], wire byte order; unused without csum
  uint8_t *wire;
  uint64_t len;
  int64_t off;      // block offset of the write's first byte
  int64_t seq;      // sequence number of its first packet
  uint32_t n0;      // bytes of the short first packet (0: the write starts on the chunk grid)
  uint32_t npk;     // packets, the empty last one of `finish` included
  uint32_t hb;      // header bytes ahead of a packet's CRCs (outpkt::out_header_bytes)
  uint32_t proto;
  uint32_t csum;    // 1: 4 CRC bytes per chunk
  uint32_t finish;  // 1: packet npk - 1 is the empty lastPacketInBlock packet
  uint32_t slices;  // workgroups per packet
};

struct Pkt {
  uint64_t wire_off;  // first byte of the packet in the stream
  uint64_t data_off;
  int64_t off, seq;
  uint32_t dlen, ncrc, cidx;  // data bytes; CRCs, the first one's index in Write::crc
  uint32_t last;
};

// Packet i of the write: packet 0 is the short first packet when n0 > 0; body
// packet j starts n0 + j * 64 KiB into the write (the one after the last data
// byte is the empty packet of `finish`).  wire.cpp checks every packet of
// every call against outpkt::plan_out_packets, the definition.
__host__ __device__ inline Pkt packet_at(const Write &w, uint32_t i) {
  const uint32_t k0 = w.n0 ? 1u : 0u;
  Pkt p;
  p.seq = w.seq + int64_t(i);
  p.last = (w.finish && i + 1u == w.npk) ? 1u : 0u;
  if (i < k0) {
    p.wire_off = 0;
    p.data_off = 0;
    p.dlen = w.n0;
    p.cidx = 0;
  } else {
    const uint64_t j = i - k0, body = w.len - w.n0;  // body: bytes on the 512-B grid
    const uint64_t at = j * kPacket < body ? j * kPacket : body;
    const uint64_t chunks = (at + kChunk - 1) / kChunk;  // grid chunks ahead of the packet
    p.data_off = w.n0 + at;
    p.dlen = uint32_t(body - at < kPacket ? body - at : kPacket);
    p.cidx = k0 + uint32_t(chunks);
    p.wire_off = (k0 ? uint64_t(w.hb) + 4u * w.csum + w.n0 : 0u) + j * w.hb + 4u * w.csum * chunks + at;
  }
  p.off = w.off + int64_t(p.data_off);
  p.ncrc = w.csum ? (p.dlen + kChunk - 1) / kChunk : 0u;
  return p;
}

// Writes wire[0, wire_len) of the write: w.npk * w.slices workgroups of 256.
// sc1: the 16-B stores are write-through (a measurement; the product uses
// one policy, wire.cpp).
hipError_t launch_frame_packets(const Write &w, bool sc1, hipStream_t stream);

}  // namespace hdfs_wire

#endif  // HADOOFUS_WIRE_INTERNAL_H
