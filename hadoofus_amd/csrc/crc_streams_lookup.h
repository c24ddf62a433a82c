// The arithmetic of libhadoofus_crc_streams.so, written once for host and
// device: fold_packets_kernel and reduce_entries_kernel
// (crc_streams_kernels.hip) run it on the streams in device memory,
// tests/consumer/crc_streams_selftest.cpp runs the same functions lane by lane
// on host-built streams against a byte-wise CRC.  Integer arithmetic only: no
// HIP header is needed to compile it.
//
// A CRC is a polynomial over GF(2) in the reflected form the main library
// keeps it in: x^0 at bit 31, so the polynomial 1 is 0x80000000 (kOne).
// Appending n zero bytes to a message multiplies its CRC by x^(8n) mod P
// (crc32c_tables.h's zeros_op is the same map as a matrix), hence
//   c(A || B) = c(A) * x^(8 |B|)  ^  c(B)
// for the CRCs as HDFS stores them (init and final inversion cancel, as in
// zlib's crc32_combine), and a block's CRC is the XOR over its chunks of
// c_i * x^(8 * bytes behind chunk i).
//
// THE FOLD.  A packet of dlen data bytes holds ncrc = ceil(dlen / cs) CRCs:
// front = ncrc - 1 chunks of cs bytes, and a last one of last_len = dlen - cs *
// front bytes (1 .. cs).  The front chunks are put flush against the end of a
// whole number of 64-lane steps (pad empty places ahead of chunk 0), so that
// lane l always stands 63 - l chunks ahead of its step's end:
//   a_l   = Horner over the steps:  a_l * x^(8 cs 64)  ^  c[64 s + l - pad]
//   F     = XOR_l  a_l * x^(8 cs (63 - l))            (kMultLane, one word a lane)
//   c_pkt = F * x^(8 last_len)  ^  c[ncrc - 1]
// One multiply a chunk behind the first step, one a lane, two a packet.
//
// THE REDUCE.  An entry's packets are dealt to the 64 lanes in contiguous runs
// (run_first, run_count); a lane runs Horner's scheme over its run,
//   acc = acc * x^(8 dlen_p)  ^  c_p,
// and is then advanced past the bytes behind its run (advance: square and
// multiply over the 64 words x^(8 * 2^b)); the XOR of the lanes is the entry's
// CRC.
#ifndef HADOOFUS_CRC_STREAMS_LOOKUP_H
#define HADOOFUS_CRC_STREAMS_LOOKUP_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_CRC_STREAMS_HD __host__ __device__ inline
#else
#define HDFS_CRC_STREAMS_HD inline
#endif

namespace hdfs_crc_streams {

constexpr uint32_t kOne = 0x80000000u;  // the polynomial 1
constexpr uint32_t kLanes = 64;
constexpr uint32_t kNoChunk = 0xFFFFFFFFu;
constexpr uint32_t kTailPackets = 3;  // read_batch_layout.h's kMaxTail

// The multiplier table of one (checksum type, chunk size), uint32 words:
constexpr uint32_t kMultLane = 0;    // [l], l < 64: x^(8 cs (63 - l))
constexpr uint32_t kMultStep = 64;   // x^(8 cs 64)
constexpr uint32_t kMultPoly = 65;   // the reflected polynomial
constexpr uint32_t kMultChunk = 66;  // cs
constexpr uint32_t kMultPow2 = 68;   // [b], b < 64: x^(8 * 2^b)
constexpr uint32_t kMultWords = 132;

// a * b mod P, branch-free: bit 31 - i of a is its x^i coefficient; b steps
// through b * x^i.
HDFS_CRC_STREAMS_HD uint32_t mulmod(uint32_t a, uint32_t b, uint32_t poly) {
  uint32_t p = 0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 31; i >= 0; i--) {
    p ^= b & (0u - ((a >> i) & 1u));
    b = (b >> 1) ^ (poly & (0u - (b & 1u)));
  }
  return p;
}

// A CRC as it stands in the stream (big-endian), loaded as a little-endian word.
HDFS_CRC_STREAMS_HD uint32_t from_wire(uint32_t w) {
  return (w >> 24) | ((w >> 8) & 0x0000FF00u) | ((w << 8) & 0x00FF0000u) | (w << 24);
}

// x^(8n) mod P from pow2[b] = x^(8 * 2^b): at most 64 trips, whatever n is.
template <class P>
HDFS_CRC_STREAMS_HD uint32_t xpow8(P pow2, uint64_t n, uint32_t poly) {
  uint32_t r = kOne;
  for (uint32_t b = 0; n; b++, n >>= 1)
    if (n & 1u) r = r == kOne ? pow2[b] : mulmod(r, pow2[b], poly);
  return r;
}

// v * x^(8n): v's message followed by n more bytes.
template <class P>
HDFS_CRC_STREAMS_HD uint32_t advance(P pow2, uint32_t v, uint64_t n, uint32_t poly) {
  for (uint32_t b = 0; n; b++, n >>= 1)
    if (n & 1u) v = mulmod(v, pow2[b], poly);
  return v;
}

// ---- the fold of a packet's CRC region ------------------------------------------------
struct Chunks {
  uint32_t front;     // chunks of cs bytes ahead of the last one
  uint32_t last_len;  // bytes of the last chunk (0: the packet has no CRC)
  uint32_t steps;     // 64-lane steps over the front chunks
  uint32_t pad;       // empty places ahead of chunk 0 in step 0
};

// ncrc == ceil(dlen / cs), as every framing-clean packet has it.
HDFS_CRC_STREAMS_HD Chunks chunks_of(uint32_t ncrc, uint32_t dlen, uint32_t cs) {
  Chunks c;
  c.front = ncrc ? ncrc - 1u : 0u;
  c.last_len = ncrc ? uint32_t(uint64_t(dlen) - uint64_t(cs) * c.front) : 0u;
  c.steps = (c.front + kLanes - 1u) / kLanes;
  c.pad = c.steps * kLanes - c.front;
  return c;
}

// The front chunk lane `lane` takes in step `step`, or kNoChunk.
HDFS_CRC_STREAMS_HD uint32_t chunk_at(const Chunks &c, uint32_t step, uint32_t lane) {
  const uint32_t j = step * kLanes + lane;
  return j >= c.pad ? j - c.pad : kNoChunk;
}

// A lane's step: `wire` is its chunk's CRC as loaded (0 where it has none).
HDFS_CRC_STREAMS_HD uint32_t fold_step(uint32_t a, uint32_t wire, uint32_t step, uint32_t mstep, uint32_t poly) {
  return (step ? mulmod(a, mstep, poly) : 0u) ^ from_wire(wire);
}

// The packet's CRC from the XOR of the lanes' a_l * kMultLane[l] (0 without
// front chunks), the last chunk's CRC as loaded and x^(8 last_len).
HDFS_CRC_STREAMS_HD uint32_t packet_crc(const Chunks &c, uint32_t front, uint32_t last_wire, uint32_t xlast,
                                        uint32_t poly) {
  if (!c.last_len) return 0u;
  return (c.front ? mulmod(front, xlast, poly) : 0u) ^ from_wire(last_wire);
}

// ---- the reduce of an entry's packets ----------------------------------------------------
// A regular entry's data lengths: nbody packets of dlen0, then ntail of their own.
struct Shape {
  uint32_t nbody, ntail, dlen0;
  uint32_t tail0, tail1, tail2;
};

HDFS_CRC_STREAMS_HD uint32_t tail_dlen(const Shape &s, uint32_t t) { return t == 0u ? s.tail0 : t == 1u ? s.tail1 : s.tail2; }

// Payload bytes of packets [0, i), i <= nbody + ntail.
HDFS_CRC_STREAMS_HD uint64_t bytes_before(const Shape &s, uint32_t i) {
  if (i <= s.nbody) return uint64_t(i) * s.dlen0;
  const uint32_t t = i - s.nbody;
  return uint64_t(s.nbody) * s.dlen0 + s.tail0 + (t > 1u ? s.tail1 : 0u) + (t > 2u ? s.tail2 : 0u);
}

// Lane `lane`'s run of npk packets: the first npk % 64 lanes take one more.
HDFS_CRC_STREAMS_HD uint32_t run_count(uint32_t npk, uint32_t lane) {
  return npk / kLanes + (lane < npk % kLanes ? 1u : 0u);
}
HDFS_CRC_STREAMS_HD uint32_t run_first(uint32_t npk, uint32_t lane) {
  const uint32_t q = npk / kLanes, r = npk % kLanes;
  return lane * q + (lane < r ? lane : r);
}

}  // namespace hdfs_crc_streams

#endif  // HADOOFUS_CRC_STREAMS_LOOKUP_H
