// Host side of wire_fused_crc.h: the compact tables of one polynomial, built
// from crc32c_tables.h (no polynomial constant and no table arithmetic of its
// own), and the image the lanes read, expanded from them.  Host only, no HIP:
// wire_fused.cpp uploads the compact tables, the selftest builds the image.
#ifndef HADOOFUS_WIRE_FUSED_TABLES_H
#define HADOOFUS_WIRE_FUSED_TABLES_H

#include <vector>

#include "crc32c_tables.h"
#include "wire_fused_crc.h"

namespace hdfs_wire_fused {
namespace crc {

// out[0, kCompactWords): the tables of polynomial `poly`.
inline void make_compact(uint32_t poly, uint32_t *out) {
  using namespace hdfs_crc32c;
  make_slicing4(reinterpret_cast<uint32_t(*)[256]>(out + kCompactSlice), poly);
  for (uint32_t j = 1; j < kPieces; j++)
    zeros_byte_tables(zeros_op(uint64_t(kPieceBytes) * j, poly), out + kCompactZ + (j - 1u) * 1024u);
  const Gf2 z1 = zeros_op(1, poly);
  uint32_t v = 0xFFFFFFFFu;
  for (uint32_t n = 0; n <= kChunkBytes; n++, v = z1.apply(v)) out[kCompactInit + n] = v;
}

// The image of wire_fused_crc.h from a polynomial's compact tables.
inline std::vector<uint32_t> make_image(const uint32_t *compact) {
  std::vector<uint32_t> img(kImageWords);
  for (uint32_t w = 0; w < kImageWords; w++) img[w] = image_word(compact, w);
  return img;
}

}  // namespace crc
}  // namespace hdfs_wire_fused

#endif  // HADOOFUS_WIRE_FUSED_TABLES_H
