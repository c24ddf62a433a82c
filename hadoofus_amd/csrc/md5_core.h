// MD5 (RFC 1321) round code, written once for the host and the device so the
// host MD5 of libhadoofus_md5crc.so and its kernel cannot drift apart.
//
// md5_block() is the compression function over sixteen little-endian message
// words.  Its shape is chosen for gfx950's VALU: the serial chain of one step
// is  t = a + f(b, c, d) + (K[i] + M[g]);  b' = b + rotl(t, s)  -- the
// (K[i] + M[g]) sums depend on the message only, so they are formed off the
// chain, and the chain itself is one bit-select or three-input xor
// (v_bfi_b32 / v_xor3_b32), one three-input add (v_add3_u32), one rotate
// (v_alignbit_b32) and one add per step.
#ifndef HADOOFUS_MD5_CORE_H
#define HADOOFUS_MD5_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_MD5_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HDFS_MD5_HD inline
#endif

namespace hdfs_md5crc {

HDFS_MD5_HD uint32_t md5_rotl(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }  // 0 < s < 32
// (b & c) | (~b & d): a bit-select of c / d by b
HDFS_MD5_HD uint32_t md5_f(uint32_t b, uint32_t c, uint32_t d) { return d ^ (b & (c ^ d)); }
// (b & d) | (c & ~d): a bit-select of b / c by d
HDFS_MD5_HD uint32_t md5_g(uint32_t b, uint32_t c, uint32_t d) { return c ^ (d & (b ^ c)); }
HDFS_MD5_HD uint32_t md5_h(uint32_t b, uint32_t c, uint32_t d) { return b ^ c ^ d; }
HDFS_MD5_HD uint32_t md5_i(uint32_t b, uint32_t c, uint32_t d) { return c ^ (b | ~d); }

HDFS_MD5_HD void md5_init(uint32_t st[4]) {
  st[0] = 0x67452301u;
  st[1] = 0xefcdab89u;
  st[2] = 0x98badcfeu;
  st[3] = 0x10325476u;
}

// One step: a = b + rotl(a + fn(b, c, d) + km, s), km = K[i] + M[g].
#define HDFS_MD5_STEP(fn, a, b, c, d, g, k, s) \
  a = b + md5_rotl(a + fn(b, c, d) + (uint32_t(k) + m[g]), s)

// st += MD5 compression of the sixteen little-endian words m[0..15].
HDFS_MD5_HD void md5_block(uint32_t st[4], const uint32_t m[16]) {
  uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
  HDFS_MD5_STEP(md5_f, a, b, c, d, 0, 0xd76aa478, 7);
  HDFS_MD5_STEP(md5_f, d, a, b, c, 1, 0xe8c7b756, 12);
  HDFS_MD5_STEP(md5_f, c, d, a, b, 2, 0x242070db, 17);
  HDFS_MD5_STEP(md5_f, b, c, d, a, 3, 0xc1bdceee, 22);
  HDFS_MD5_STEP(md5_f, a, b, c, d, 4, 0xf57c0faf, 7);
  HDFS_MD5_STEP(md5_f, d, a, b, c, 5, 0x4787c62a, 12);
  HDFS_MD5_STEP(md5_f, c, d, a, b, 6, 0xa8304613, 17);
  HDFS_MD5_STEP(md5_f, b, c, d, a, 7, 0xfd469501, 22);
  HDFS_MD5_STEP(md5_f, a, b, c, d, 8, 0x698098d8, 7);
  HDFS_MD5_STEP(md5_f, d, a, b, c, 9, 0x8b44f7af, 12);
  HDFS_MD5_STEP(md5_f, c, d, a, b, 10, 0xffff5bb1, 17);
  HDFS_MD5_STEP(md5_f, b, c, d, a, 11, 0x895cd7be, 22);
  HDFS_MD5_STEP(md5_f, a, b, c, d, 12, 0x6b901122, 7);
  HDFS_MD5_STEP(md5_f, d, a, b, c, 13, 0xfd987193, 12);
  HDFS_MD5_STEP(md5_f, c, d, a, b, 14, 0xa679438e, 17);
  HDFS_MD5_STEP(md5_f, b, c, d, a, 15, 0x49b40821, 22);

  HDFS_MD5_STEP(md5_g, a, b, c, d, 1, 0xf61e2562, 5);
  HDFS_MD5_STEP(md5_g, d, a, b, c, 6, 0xc040b340, 9);
  HDFS_MD5_STEP(md5_g, c, d, a, b, 11, 0x265e5a51, 14);
  HDFS_MD5_STEP(md5_g, b, c, d, a, 0, 0xe9b6c7aa, 20);
  HDFS_MD5_STEP(md5_g, a, b, c, d, 5, 0xd62f105d, 5);
  HDFS_MD5_STEP(md5_g, d, a, b, c, 10, 0x02441453, 9);
  HDFS_MD5_STEP(md5_g, c, d, a, b, 15, 0xd8a1e681, 14);
  HDFS_MD5_STEP(md5_g, b, c, d, a, 4, 0xe7d3fbc8, 20);
  HDFS_MD5_STEP(md5_g, a, b, c, d, 9, 0x21e1cde6, 5);
  HDFS_MD5_STEP(md5_g, d, a, b, c, 14, 0xc33707d6, 9);
  HDFS_MD5_STEP(md5_g, c, d, a, b, 3, 0xf4d50d87, 14);
  HDFS_MD5_STEP(md5_g, b, c, d, a, 8, 0x455a14ed, 20);
  HDFS_MD5_STEP(md5_g, a, b, c, d, 13, 0xa9e3e905, 5);
  HDFS_MD5_STEP(md5_g, d, a, b, c, 2, 0xfcefa3f8, 9);
  HDFS_MD5_STEP(md5_g, c, d, a, b, 7, 0x676f02d9, 14);
  HDFS_MD5_STEP(md5_g, b, c, d, a, 12, 0x8d2a4c8a, 20);

  HDFS_MD5_STEP(md5_h, a, b, c, d, 5, 0xfffa3942, 4);
  HDFS_MD5_STEP(md5_h, d, a, b, c, 8, 0x8771f681, 11);
  HDFS_MD5_STEP(md5_h, c, d, a, b, 11, 0x6d9d6122, 16);
  HDFS_MD5_STEP(md5_h, b, c, d, a, 14, 0xfde5380c, 23);
  HDFS_MD5_STEP(md5_h, a, b, c, d, 1, 0xa4beea44, 4);
  HDFS_MD5_STEP(md5_h, d, a, b, c, 4, 0x4bdecfa9, 11);
  HDFS_MD5_STEP(md5_h, c, d, a, b, 7, 0xf6bb4b60, 16);
  HDFS_MD5_STEP(md5_h, b, c, d, a, 10, 0xbebfbc70, 23);
  HDFS_MD5_STEP(md5_h, a, b, c, d, 13, 0x289b7ec6, 4);
  HDFS_MD5_STEP(md5_h, d, a, b, c, 0, 0xeaa127fa, 11);
  HDFS_MD5_STEP(md5_h, c, d, a, b, 3, 0xd4ef3085, 16);
  HDFS_MD5_STEP(md5_h, b, c, d, a, 6, 0x04881d05, 23);
  HDFS_MD5_STEP(md5_h, a, b, c, d, 9, 0xd9d4d039, 4);
  HDFS_MD5_STEP(md5_h, d, a, b, c, 12, 0xe6db99e5, 11);
  HDFS_MD5_STEP(md5_h, c, d, a, b, 15, 0x1fa27cf8, 16);
  HDFS_MD5_STEP(md5_h, b, c, d, a, 2, 0xc4ac5665, 23);

  HDFS_MD5_STEP(md5_i, a, b, c, d, 0, 0xf4292244, 6);
  HDFS_MD5_STEP(md5_i, d, a, b, c, 7, 0x432aff97, 10);
  HDFS_MD5_STEP(md5_i, c, d, a, b, 14, 0xab9423a7, 15);
  HDFS_MD5_STEP(md5_i, b, c, d, a, 5, 0xfc93a039, 21);
  HDFS_MD5_STEP(md5_i, a, b, c, d, 12, 0x655b59c3, 6);
  HDFS_MD5_STEP(md5_i, d, a, b, c, 3, 0x8f0ccc92, 10);
  HDFS_MD5_STEP(md5_i, c, d, a, b, 10, 0xffeff47d, 15);
  HDFS_MD5_STEP(md5_i, b, c, d, a, 1, 0x85845dd1, 21);
  HDFS_MD5_STEP(md5_i, a, b, c, d, 8, 0x6fa87e4f, 6);
  HDFS_MD5_STEP(md5_i, d, a, b, c, 15, 0xfe2ce6e0, 10);
  HDFS_MD5_STEP(md5_i, c, d, a, b, 6, 0xa3014314, 15);
  HDFS_MD5_STEP(md5_i, b, c, d, a, 13, 0x4e0811a1, 21);
  HDFS_MD5_STEP(md5_i, a, b, c, d, 4, 0xf7537e82, 6);
  HDFS_MD5_STEP(md5_i, d, a, b, c, 11, 0xbd3af235, 10);
  HDFS_MD5_STEP(md5_i, c, d, a, b, 2, 0x2ad7d2bb, 15);
  HDFS_MD5_STEP(md5_i, b, c, d, a, 9, 0xeb86d391, 21);
  st[0] += a;
  st[1] += b;
  st[2] += c;
  st[3] += d;
}

#undef HDFS_MD5_STEP

// Number of 64-byte MD5 blocks of a message of nwords 32-bit words: the
// words, the 0x80 word and the two length words, rounded up.
HDFS_MD5_HD uint64_t md5_words_blocks(uint64_t nwords) { return (nwords + 3 + 15) / 16; }

}  // namespace hdfs_md5crc

#endif  // HADOOFUS_MD5_CORE_H
