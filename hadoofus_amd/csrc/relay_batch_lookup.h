// The arithmetic of libhadoofus_relay_batch.so that is its own, written once
// for host and device: relay_fused_batch_kernel (relay_batch_kernels.hip) runs
// it on the scalar unit, relay_batch.cpp sizes a write's stream with it, and
// tests/consumer/relay_batch_selftest.cpp runs the same functions against a
// per-byte model of a frame_step walk.  Plain integers; no HIP header is needed
// to compile it.
//
// THE INPUT is a regular read stream (read_batch_layout.h): K data packets of
// dlen0 bytes (a multiple of 512, at most 65536) a stride apart, at most one
// shorter data packet behind them and at most one empty last packet (Geom).
// THE OUTPUT is the stream of a write that starts on the 512-B chunk grid: data
// packets of 65536 bytes, the last one shorter, and the empty last packet of
// `finish` (out_shape; the packets' places are wire_internal.h's packet_at).
//
// Both sides cut the payload into the same 512-B chunks.  Payload chunk q lies
// in input data packet q / (dlen0 / 512) while that is below K, else in the
// shorter packet; a packet's header, its CRC words and its data follow each
// other, so the chunk's bytes and its CRC word have a place in the stream that
// follows from the Geom alone (seek, next_chunk, data_at, crc_at).  A wave's
// round of an output packet is eight payload chunks from a multiple of eight:
// where dlen0 is no multiple of 4096 the round spans several input packets, but
// every seam lies between two chunks, never inside one.
//
// Every input header is compared by one workgroup: a data packet's by the one
// whose output packet holds the packet's first data byte, the empty last
// packet's by the one of the write's last output packet (first_header,
// end_header).
#ifndef HADOOFUS_RELAY_BATCH_LOOKUP_H
#define HADOOFUS_RELAY_BATCH_LOOKUP_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_RELAY_HD __host__ __device__ inline
#else
#define HDFS_RELAY_HD inline
#endif

namespace hdfs_relay_batch {

constexpr uint32_t kGrid = 512;                      // the chunk of both sides
constexpr uint32_t kOutData = 65536;                 // data bytes of an output packet
constexpr uint32_t kOutChunks = kOutData / kGrid;    // 128
constexpr uint64_t kMaxConsumed = uint64_t(1) << 32;  // one buffer range covers an entry's stream

// The input stream of a regular entry.
struct Geom {
  uint64_t stride;    // wire bytes of a full packet: hb0 + 4 cpp0 + 512 cpp0
  uint64_t short_at;  // first byte of the shorter data packet in the stream
  uint64_t payload;   // 512 K cpp0 + short_dlen
  uint32_t cpp0;      // chunks of a full packet, 1 .. 128
  uint32_t hb0;       // header bytes of a full packet
  uint32_t K;         // full packets, >= 1
  uint32_t short_dlen, short_hb;  // 0, 0: no shorter packet
  uint32_t empty;     // 1: the empty last packet ends the stream
};

HDFS_RELAY_HD uint32_t crc_words(uint32_t dlen) { return (dlen + kGrid - 1u) / kGrid; }

// ---- the output side ---------------------------------------------------------------
// The stream of a write of `payload` bytes at a block offset on the chunk grid:
// npk packets (the empty last one of `finish` included), hb header bytes each,
// a CRC word per chunk, the payload.
HDFS_RELAY_HD void out_shape(uint64_t payload, uint32_t hb, bool finish, uint64_t &wire_len, uint64_t &npk) {
  npk = (payload + kOutData - 1u) / kOutData + (finish ? 1u : 0u);
  wire_len = npk * hb + 4u * ((payload + kGrid - 1u) / kGrid) + payload;
}

// ---- where a payload chunk lies in the input -----------------------------------------
// Chunk `ch` of input data packet `ip` (ip == K: the shorter packet).
struct Cursor {
  uint32_t ip, ch;
};

// Payload chunk q (q * 512 < payload).
HDFS_RELAY_HD Cursor seek(const Geom &g, uint32_t q) {
  const uint32_t full = g.K * g.cpp0;  // < 2^23: the stream is below 4 GiB
  if (q >= full) return Cursor{g.K, q - full};
  const uint32_t ip = q / g.cpp0;
  return Cursor{ip, q - ip * g.cpp0};
}

// The payload's next chunk.
HDFS_RELAY_HD Cursor next_chunk(const Geom &g, Cursor c) {
  c.ch++;
  if (c.ip < g.K && c.ch == g.cpp0) {
    c.ip++;
    c.ch = 0;
  }
  return c;
}

HDFS_RELAY_HD uint64_t packet_start(const Geom &g, uint32_t ip) { return ip < g.K ? ip * g.stride : g.short_at; }
HDFS_RELAY_HD uint32_t packet_header(const Geom &g, uint32_t ip) { return ip < g.K ? g.hb0 : g.short_hb; }
HDFS_RELAY_HD uint32_t packet_crcs(const Geom &g, uint32_t ip) { return ip < g.K ? g.cpp0 : crc_words(g.short_dlen); }

// The stream offsets of the chunk's CRC word and of its first data byte.
HDFS_RELAY_HD uint64_t crc_at(const Geom &g, Cursor c) {
  return packet_start(g, c.ip) + packet_header(g, c.ip) + 4u * c.ch;
}
HDFS_RELAY_HD uint64_t data_at(const Geom &g, Cursor c) {
  return packet_start(g, c.ip) + packet_header(g, c.ip) + 4u * packet_crcs(g, c.ip) + uint64_t(kGrid) * c.ch;
}

// ---- which input headers an output packet's workgroup compares --------------------------
// Input packets count data packets first (0 .. K - 1, then the shorter one),
// the empty last packet behind them.
HDFS_RELAY_HD uint32_t in_data_packets(const Geom &g) { return g.K + (g.short_dlen ? 1u : 0u); }
HDFS_RELAY_HD uint32_t in_packets(const Geom &g) { return in_data_packets(g) + (g.empty ? 1u : 0u); }

// The first input data packet whose first data byte is at or behind output
// packet j's first: ceil(128 j / cpp0), at most in_data_packets.  j <= 2^16.
HDFS_RELAY_HD uint32_t first_header(const Geom &g, uint32_t j) {
  const uint32_t i = (j * kOutChunks + g.cpp0 - 1u) / g.cpp0, nd = in_data_packets(g);
  return i < nd ? i : nd;
}

// One past the last input packet output packet j < out_npk compares.
HDFS_RELAY_HD uint32_t end_header(const Geom &g, uint32_t j, uint32_t out_npk) {
  return j + 1u == out_npk ? in_packets(g) : first_header(g, j + 1u);
}

}  // namespace hdfs_relay_batch

#endif  // HADOOFUS_RELAY_BATCH_LOOKUP_H
