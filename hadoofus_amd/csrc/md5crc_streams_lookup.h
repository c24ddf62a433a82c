// Where the CRC words of a packet stream lie, written once for host and
// device: digest_streams_kernel (md5crc_streams_kernels.hip) runs it with one
// lane per entry on the descriptors in device memory;
// tests/consumer/md5crc_streams_selftest.cpp runs the same functions on
// host-built streams against a brute-force frame_step walk.  Plain integer
// arithmetic: no HIP header is needed to compile it, and nothing here reads a
// stream byte.
//
// A regular stream (read_batch_layout.h) is nbody body packets of one size, one
// stride apart, and at most three tail packets framed by the probe.  Packet
// i's CRC REGION is the 4 * ceil(dlen / 512) bytes behind its header: body
// packet i's at i * stride + hb0, wpp = dlen0 / 512 words; a tail packet's at
// its own offset, ceil(dlen / 512) words, none for the empty last packet.  The
// MD5CRC message is the regions' concatenation in packet order, nwords words.
//
// The CURSOR walks that message a word at a time without a division: `off` is
// the next word's byte offset in the stream, `left` the words that remain in
// its region, `pkt` the region's packet.  When a region is used up the next one
// follows by one addition (body) or from the tail table; a region of no words
// is passed over.  An MD5 block is sixteen words: when the cursor's region
// holds at least sixteen more the block is one span of 64 bytes (take_span, the
// kernel's four wide loads), else it is taken word by word (take_word) and may
// begin in one packet and end in another.  Every count follows from the
// descriptor, that is from lengths: the walk makes exactly nwords steps and
// every offset it yields lies inside a region, whatever the stream's bytes are.
//
// A stream lies at any byte address, so a word does too.  Global loads of the
// device want 4-byte alignment, so a word at address A = base + off with a = A
// & 3 != 0 is made of the two aligned words around it (join); where the second
// of them would reach past the bytes the walk may read (`limit`, the entry's
// consumed bytes) the word is read byte by byte instead (by_bytes).  A block is
// kept as loaded (Loaded) and joined only when MD5 takes it (message_words).
#ifndef HADOOFUS_MD5CRC_STREAMS_LOOKUP_H
#define HADOOFUS_MD5CRC_STREAMS_LOOKUP_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_MD5CRC_STREAMS_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HDFS_MD5CRC_STREAMS_HD inline
#endif

// The loop over a block's words has constant bounds and is unrolled on the
// device, so that the words stay in registers.
#if defined(__clang__)
#define HDFS_MD5CRC_STREAMS_UNROLL _Pragma("unroll")
#else
#define HDFS_MD5CRC_STREAMS_UNROLL
#endif

namespace hdfs_md5crc_streams {

constexpr uint32_t kTailRegions = 3;  // read_batch_layout.h's kMaxTail
constexpr uint32_t kBlockWords = 16;  // one MD5 block

// The CRC regions of one entry.  base: the stream's address (or, for an entry
// that took the fallback, the library's scratch where its CRCs were gathered:
// no body, one tail region).
struct Regions {
  uint64_t base;
  uint64_t limit;   // bytes from base on that may be read
  uint64_t stride;  // wire bytes of a body packet
  uint64_t nwords;  // CRC words of all regions: the message is 4 * nwords bytes
  uint64_t tail_off0, tail_off1, tail_off2;        // named, not an array: they stay in registers
  uint32_t tail_words0, tail_words1, tail_words2;  // 0 from ntail on
  uint32_t hb0;    // header bytes ahead of a body packet's CRCs
  uint32_t wpp;    // CRC words of a body packet (>= 1 when nbody > 0)
  uint32_t nbody;  // body packets
  uint32_t ntail;  // tail regions in use
  uint32_t nblk;   // MD5 blocks of the message (md5_core.h: md5_words_blocks(nwords))
  uint32_t entry;  // index in the batch
};

struct Cursor {
  uint64_t off;     // the next word's byte offset from base
  uint64_t pk_off;  // the current body packet's region, its first byte
  uint32_t left;    // words left in the current region
  uint32_t pkt;     // the current region's packet: < nbody body, else tail pkt - nbody
};

// The words of all regions; what the probe stores as nwords.
HDFS_MD5CRC_STREAMS_HD uint64_t count_words(const Regions &r) {
  return uint64_t(r.nbody) * r.wpp + r.tail_words0 + r.tail_words1 + r.tail_words2;
}

// Tail region t; past the last one: nothing.
HDFS_MD5CRC_STREAMS_HD void tail_region(const Regions &r, uint32_t t, uint64_t &off, uint32_t &words) {
  // values first, then the choice: a choice between the fields themselves is an
  // address, and the descriptor would have to live in memory for it
  const uint64_t o0 = r.tail_off0, o1 = r.tail_off1, o2 = r.tail_off2;
  const uint32_t w0 = r.tail_words0, w1 = r.tail_words1, w2 = r.tail_words2;
  off = t == 0u ? o0 : t == 1u ? o1 : o2;
  words = t == 0u ? w0 : t == 1u ? w1 : w2;
  if (t >= r.ntail || t >= kTailRegions) words = 0u;
}

// On region 0, which may be empty: settle() before a word is taken.
HDFS_MD5CRC_STREAMS_HD Cursor start(const Regions &r) {
  Cursor c;
  c.pkt = 0u;
  c.pk_off = r.hb0;
  if (r.nbody) {
    c.off = c.pk_off;
    c.left = r.wpp;
  } else {
    tail_region(r, 0u, c.off, c.left);
  }
  return c;
}

// The next region, by one addition or from the tail table.
HDFS_MD5CRC_STREAMS_HD void next_region(const Regions &r, Cursor &c) {
  c.pkt++;
  if (c.pkt < r.nbody) {
    c.pk_off += r.stride;
    c.off = c.pk_off;
    c.left = r.wpp;
  } else {
    tail_region(r, c.pkt - r.nbody, c.off, c.left);
  }
}

// Passes over used-up and empty regions: afterwards left > 0 whenever a word of
// the message is still ahead.  At most kTailRegions + 1 steps (a body region is
// never empty), so the loop is bounded whatever the descriptor holds.
HDFS_MD5CRC_STREAMS_HD void settle(const Regions &r, Cursor &c) {
  for (uint32_t s = 0; s <= kTailRegions && c.left == 0u; s++) next_region(r, c);
}

// Whether the next sixteen words are one span of 64 bytes of the current region.
HDFS_MD5CRC_STREAMS_HD bool span_ahead(const Cursor &c) { return c.left >= kBlockWords; }

// That span's offset; the cursor moves behind it.
HDFS_MD5CRC_STREAMS_HD uint64_t take_span(Cursor &c) {
  const uint64_t off = c.off;
  c.off += 4u * kBlockWords;
  c.left -= kBlockWords;
  return off;
}

// The next word's offset (a word must be ahead); the cursor moves behind it.
HDFS_MD5CRC_STREAMS_HD uint64_t take_word(const Regions &r, Cursor &c) {
  settle(r, c);
  const uint64_t off = c.off;
  c.off += 4u;
  c.left = c.left ? c.left - 1u : 0u;
  return off;
}

// ---- a word at any byte address ---------------------------------------------------
// The word at A from the aligned words lo at A - a and hi at A - a + 4, a = A & 3
// (little-endian; a == 0: lo itself).
HDFS_MD5CRC_STREAMS_HD uint32_t join(uint32_t lo, uint32_t hi, uint32_t a) {
  return uint32_t(((uint64_t(hi) << 32) | lo) >> (8u * a));
}

// n consecutive words at base + off, misaligned by a != 0, want the n + 1
// aligned words from base + off - a on; the last of them ends at
// off - a + 4 (n + 1).  False: it would reach past limit, read the bytes.
HDFS_MD5CRC_STREAMS_HD bool aligned_cover_ok(const Regions &r, uint64_t off, uint32_t a, uint32_t n) {
  return off >= a && off - a + 4u * (uint64_t(n) + 1u) <= r.limit;
}

HDFS_MD5CRC_STREAMS_HD uint32_t by_bytes(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) {
  return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// ---- the sixteen words of an MD5 block ----------------------------------------------
// A block AS LOADED: word j is join(lo[j], hi[j], a_j), a_j two bits of sh.
// The kernel fills one before the MD5 rounds of the block ahead and joins it
// behind them (message_words), so that no loaded register is touched before the
// rounds and the loads' latency hides under them.
struct Loaded {
  uint32_t lo[kBlockWords], hi[kBlockWords];
  uint32_t sh;  // word j's misalignment in bits 2 j, 2 j + 1
};

// Where the two aligned words around the word at address A lie: A - a, and
// A - a + 4 -- or, for an aligned word, the same word again, so that nothing
// behind it is read.
HDFS_MD5CRC_STREAMS_HD uint64_t lo_address(uint64_t A) { return A & ~uint64_t(3); }
HDFS_MD5CRC_STREAMS_HD uint64_t hi_address(uint64_t A) { return (A & ~uint64_t(3)) + ((A & 3u) ? 4u : 0u); }

HDFS_MD5CRC_STREAMS_HD void message_words(const Loaded &x, uint32_t m[kBlockWords]) {
  HDFS_MD5CRC_STREAMS_UNROLL
  for (uint32_t j = 0; j < kBlockWords; j++) m[j] = join(x.lo[j], x.hi[j], (x.sh >> (2u * j)) & 3u);
}

// Block blk of the message, as MD5 takes it once joined: the message's words (a
// CRC's four wire bytes, loaded little-endian, are the message word), then the
// 0x80 word, zeros behind it.  The two length words are the caller's
// (md5_core.h).  span(off, x): sixteen words at base + off into x;
// word(off, lo, hi, a): one.  Both are handed offsets inside a region only.
template <class Span, class Word>
HDFS_MD5CRC_STREAMS_HD void block_words(const Regions &r, Cursor &c, uint32_t blk, Span span, Word word, Loaded &x) {
  const uint64_t i0 = uint64_t(blk) * kBlockWords;
  if (i0 + kBlockWords <= r.nwords) {
    settle(r, c);
    if (span_ahead(c)) {
      span(take_span(c), x);
      return;
    }
  }
  x.sh = 0u;
  HDFS_MD5CRC_STREAMS_UNROLL
  for (uint32_t j = 0; j < kBlockWords; j++) {
    const uint64_t i = i0 + j;
    uint32_t lo = i == r.nwords ? 0x00000080u : 0u, hi = 0u, a = 0u;
    if (i < r.nwords) word(take_word(r, c), lo, hi, a);
    x.lo[j] = lo;
    x.hi[j] = hi;
    x.sh |= a << (2u * j);
  }
}

}  // namespace hdfs_md5crc_streams

#endif  // HADOOFUS_MD5CRC_STREAMS_LOOKUP_H
