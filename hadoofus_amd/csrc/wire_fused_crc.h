// The CRC of a 512-B chunk as libhadoofus_wire_fused.so computes it, written
// once for host and device: the table image and the arithmetic of one lane.
// frame_fused_kernel (wire_fused_kernels.hip) runs these functions on the
// image in LDS; tests/consumer/wire_fused_selftest.cpp runs the same functions
// on the same image in host memory, lane by lane of a simulated wave.
//
// A chunk is cut into eight 64-B pieces, one per lane.  Every lane runs 16
// slicing-by-4 steps over its piece from a zero register (piece_raw), shifts
// the result past the pieces behind it with Z_{64 (7 - i)} (piece_shift), the
// eight results are XORed (chunk_fold; the kernel does it with DPP), and the
// contribution of the initial register, Z_n(0xFFFFFFFF) for a chunk of n
// bytes, joins at the end with the inversion and the byte order (chunk_final).
// A chunk shorter than 512 B is right-aligned in a zero frame of 512 B first:
// leading zero bytes leave a zero register zero, so the same eight pieces give
// its CRC, and only the constant Z_n differs.
//
// The slicing tables are replicated 32 times so that lane l of a wave always
// reads bank l (no bank conflicts, as the main library's tiled kernel does):
// t_k[e] for lane l is word slice_at(k, e, l) of the image.
#ifndef HADOOFUS_WIRE_FUSED_CRC_H
#define HADOOFUS_WIRE_FUSED_CRC_H

#include <stdint.h>

#if defined(__HIPCC__)
#define HDFS_FUSED_HD __host__ __device__ inline
#else
#define HDFS_FUSED_HD inline
#endif

namespace hdfs_wire_fused {
namespace crc {

constexpr uint32_t kChunkBytes = 512, kPieceBytes = 64, kPieces = 8, kPieceWords = 16;

// ---- the compact tables (device global memory; one set per polynomial) --------
// [0, 1024)      t[k * 256 + e]: byte e followed by k zero bytes (make_slicing4)
// [1024, 8192)   Z_{64 j}, j = 1..7, as 4 x 256 byte tables (zeros_byte_tables)
// [8192, 8705)   Z_n(0xFFFFFFFF), n = 0..512
constexpr uint32_t kCompactSlice = 0, kCompactZ = 1024, kCompactInit = 8192, kCompactWords = 8192 + 513;

// ---- the image (LDS; the same words in host memory for the selftest) -----------
// [0, 32768)      the slicing tables, 32 replicas: slice_at()
// [32768, 39936)  Z_{64 j}, j = 1..7, unreplicated (four reads a round)
constexpr uint32_t kReplicas = 32, kImageZ = 1024 * kReplicas, kImageWords = kImageZ + 7 * 1024;

// Word of t_k[e] that lane `lane` reads: tables 3 and 2 share the first 64 KiB,
// 1 and 0 the second; an entry of a pair is 64 words, 32 lanes of each table.
HDFS_FUSED_HD uint32_t slice_at(uint32_t k, uint32_t e, uint32_t lane) {
  return ((3u - k) >> 1) * 16384u + e * 64u + ((3u - k) & 1u) * 32u + (lane & 31u);
}

// compact[0, 8192) -> image word w (the kernel's fill and the host's).
HDFS_FUSED_HD uint32_t image_word(const uint32_t *compact, uint32_t w) {
  if (w >= kImageZ) return compact[kCompactZ + (w - kImageZ)];
  const uint32_t pair = w >> 14, e = (w >> 6) & 255u, odd = (w >> 5) & 1u;
  return compact[kCompactSlice + (3u - (2u * pair + odd)) * 256u + e];
}

// One slicing-by-4 step: the register after the four bytes of x = register ^ word.
HDFS_FUSED_HD uint32_t slice_step(const uint32_t *img, uint32_t lane, uint32_t x) {
  return img[slice_at(3, x & 0xffu, lane)] ^ img[slice_at(2, (x >> 8) & 0xffu, lane)] ^
         img[slice_at(1, (x >> 16) & 0xffu, lane)] ^ img[slice_at(0, x >> 24, lane)];
}

// A piece's raw register from its 64 bytes (16 little-endian words), from zero.
HDFS_FUSED_HD uint32_t piece_raw(const uint32_t *img, uint32_t lane, const uint32_t (&w)[kPieceWords]) {
  uint32_t r = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (uint32_t j = 0; j < kPieceWords; j++) r = slice_step(img, lane, r ^ w[j]);
  return r;
}

// The shift of piece i's register past the rest of its chunk: Z_{64 (7 - i)}.
HDFS_FUSED_HD uint32_t piece_shift(const uint32_t *img, uint32_t i, uint32_t r) {
  if (i >= kPieces - 1u) return r;
  const uint32_t *z = img + kImageZ + (6u - i) * 1024u;
  return z[r & 0xffu] ^ z[256u + ((r >> 8) & 0xffu)] ^ z[512u + ((r >> 16) & 0xffu)] ^ z[768u + (r >> 24)];
}

// The fold of a chunk's shifted pieces.
HDFS_FUSED_HD uint32_t chunk_fold(const uint32_t (&s)[kPieces]) {
  return s[0] ^ s[1] ^ s[2] ^ s[3] ^ s[4] ^ s[5] ^ s[6] ^ s[7];
}

// The chunk's CRC as the dword whose little-endian store is its four wire
// (big-endian) bytes: init = Z_n(0xFFFFFFFF), n the chunk's bytes.
HDFS_FUSED_HD uint32_t chunk_final(uint32_t fold, uint32_t init) {
  const uint32_t c = ~(fold ^ init);
  return (c >> 24) | ((c >> 8) & 0xff00u) | ((c << 8) & 0xff0000u) | (c << 24);
}

}  // namespace crc
}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_CRC_H
