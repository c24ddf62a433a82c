// Shared between writev.cpp (host entry points) and writev_kernels.hip.
#ifndef HADOOFUS_WRITEV_INTERNAL_H
#define HADOOFUS_WRITEV_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hdfs_writev {

// One piece of a gathered chunk: len > 0 bytes at p, inside one fragment.
struct Piece {
  const uint8_t *p;
  uint32_t len;
  uint32_t pad;
};
static_assert(sizeof(Piece) == 16, "Piece layout");

// One gathered chunk: its CRC goes to crcs[slot]; its bytes are pieces
// [first, first + count) of the piece table, in order.
struct GChunk {
  uint32_t slot;
  uint32_t first;
  uint32_t count;
  uint32_t pad;
};
static_assert(sizeof(GChunk) == 16, "GChunk layout");

constexpr uint32_t kSliceWords = 4 * 256;  // slicing-by-4 tables t0..t3 of one polynomial

// crcs[ch[g].slot] = big-endian CRC (init 0, pre / post inversion inside) of
// gathered chunk g, chained over its pieces; one lane per chunk.  tab: device
// u32[kSliceWords] of the polynomial wanted.  A descriptor that points
// outside the tables (first + count > npieces, slot >= nchunks) is skipped.
hipError_t launch_gather_chunks(const GChunk *ch, uint32_t ngathered, const Piece *pc, uint32_t npieces,
                                const uint32_t *tab, uint32_t *crcs, uint32_t nchunks, hipStream_t stream);

}  // namespace hdfs_writev

#endif  // HADOOFUS_WRITEV_INTERNAL_H
