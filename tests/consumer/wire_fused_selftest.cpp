// Stand-alone check of the fused wire library's CRC arithmetic on the CPU:
// wire_fused_crc.h's lane functions, run for every lane of a simulated wave on
// the table image wire_fused_tables.h builds, against a bitwise CRC.  Built
// with -fsanitize=address,undefined by tests/test_wire_fused_cpu.py; nothing
// of it is loaded into Python.
//
// The wave is simulated as frame_fused_kernel (wire_fused_kernels.hip) uses
// it: a round's four loads in the kernel's lane order, the two permlane swap
// stages as data movement between the 64 lanes' registers, then piece_raw,
// piece_shift, chunk_fold and chunk_final per lane; and the ragged path's
// right-aligned frame, eight bytes a lane, gathered into eight pieces.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wire_fused_tables.h"

using namespace hdfs_wire_fused::crc;

static int failures = 0;
#define CHECK(c, ...)                   \
  do {                                  \
    if (!(c)) {                         \
      failures++;                       \
      if (failures < 20) {              \
        std::printf("FAIL %s: ", #c);   \
        std::printf(__VA_ARGS__);       \
        std::printf("\n");              \
      }                                 \
    }                                   \
  } while (0)

static uint32_t bitwise(uint32_t poly, const uint8_t *p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; i++) {
    c ^= p[i];
    for (int b = 0; b < 8; b++) c = (c >> 1) ^ (poly & (0u - (c & 1u)));
  }
  return ~c;
}

// What lane 8c stores for a chunk of CRC v: the dword whose bytes in memory are v's, big-endian.
static uint32_t wire_dword(uint32_t v) {
  const uint8_t b[4] = {uint8_t(v >> 24), uint8_t(v >> 16), uint8_t(v >> 8), uint8_t(v)};
  uint32_t d;
  std::memcpy(&d, b, 4);  // the hosts this runs on and the device are little-endian
  return d;
}

static uint32_t word_at(const uint8_t *p) {
  return uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
}

struct Tables {
  std::vector<uint32_t> compact, img;
  explicit Tables(uint32_t poly) : compact(kCompactWords) {
    make_compact(poly, compact.data());
    img = make_image(compact.data());
  }
  uint32_t init(uint32_t n) const { return compact[kCompactInit + n]; }
};

// v_permlane16_swap (rows = 16 lanes: the odd rows of a trade places with the
// even rows of b) and v_permlane32_swap (the upper half of a with the lower
// half of b).
static void swap_rows(uint32_t (&reg)[64][16], int a, int b, int width) {
  for (int l = 0; l < 64; l++)
    if (!(l & width)) {
      const uint32_t t = reg[l + width][a];
      reg[l + width][a] = reg[l][b];
      reg[l][b] = t;
    }
}

// One round of the kernel: data holds nfr full chunks.  out[c]: chunk c's dword.
static void round_crcs(const Tables &t, const uint8_t *data, uint32_t nfr, uint32_t (&out)[8]) {
  static uint32_t reg[64][16];
  for (uint32_t l = 0; l < 64; l++)
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t piece = 64u * k + 4u * (l & 15u) + (l >> 4), o = 16u * piece;
      for (uint32_t c = 0; c < 4; c++)  // a piece outside the range loads zeros
        reg[l][4 * k + c] = o / kChunkBytes < nfr ? word_at(data + o + 4u * c) : 0u;
    }
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < 4; k += 2) swap_rows(reg, k * 4 + c, (k + 1) * 4 + c, 16);
  for (int c = 0; c < 4; c++)
    for (int k = 0; k < 2; k++) swap_rows(reg, k * 4 + c, (k + 2) * 4 + c, 32);
  uint32_t s[64];
  for (uint32_t l = 0; l < 64; l++) {
    // the transpose left lane l with the 64 contiguous bytes of piece l
    if (l / 8u < nfr)
      for (uint32_t j = 0; j < 16; j++)
        CHECK(reg[l][j] == word_at(data + 64u * l + 4u * j), "transpose: lane %u word %u", l, j);
    s[l] = piece_shift(t.img.data(), l & 7u, piece_raw(t.img.data(), l, reg[l]));
  }
  for (uint32_t c = 0; c < 8; c++) {
    uint32_t v[8];
    for (uint32_t i = 0; i < 8; i++) v[i] = s[8 * c + i];
    out[c] = chunk_final(chunk_fold(v), t.init(kChunkBytes));
  }
}

// The ragged path: a chunk of n <= 512 bytes right-aligned in a zero frame.
static uint32_t ragged_crc(const Tables &t, const uint8_t *data, uint32_t n) {
  const uint32_t pad = kChunkBytes - n;
  uint32_t w0[64], w1[64];
  for (uint32_t l = 0; l < 64; l++) {
    uint8_t b[8];
    for (uint32_t j = 0; j < 8; j++) {
      const uint32_t f = 8u * l + j;
      b[j] = f >= pad ? data[f - pad] : 0u;
    }
    w0[l] = word_at(b);
    w1[l] = word_at(b + 4);
  }
  uint32_t v[8];
  for (uint32_t l = 0; l < 8; l++) {  // lane l: piece l, gathered from lanes 8l .. 8l + 7
    uint32_t x[16];
    for (uint32_t j = 0; j < 8; j++) {
      x[2 * j] = w0[8 * l + j];
      x[2 * j + 1] = w1[8 * l + j];
    }
    v[l] = piece_shift(t.img.data(), l, piece_raw(t.img.data(), l, x));
  }
  return chunk_final(chunk_fold(v), t.init(n));
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint8_t next_byte() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return uint8_t(g_rng >> 32);
}

static void run(uint32_t poly, const char *name, uint32_t kat) {
  CHECK(bitwise(poly, reinterpret_cast<const uint8_t *>("123456789"), 9) == kat, "%s known answer", name);
  const Tables t(poly);
  // the image is the compact tables, replicated: every replica of every entry
  for (uint32_t k = 0; k < 4; k++)
    for (uint32_t e = 0; e < 256; e++)
      for (uint32_t l = 0; l < 64; l++)
        CHECK(t.img[slice_at(k, e, l)] == t.compact[kCompactSlice + k * 256 + e], "%s image t%u[%u] lane %u", name, k,
              e, l);
  std::vector<uint8_t> buf(4096);
  for (int fill = 0; fill < 5; fill++) {  // three random fills, all-zero, all-0xFF
    for (auto &b : buf) b = fill < 3 ? next_byte() : (fill == 3 ? 0x00 : 0xFF);
    for (uint32_t nfr = 1; nfr <= 8; nfr++) {  // 4 KiB rounds holding 1..8 chunks
      uint32_t got[8];
      round_crcs(t, buf.data(), nfr, got);
      for (uint32_t c = 0; c < nfr; c++)
        CHECK(got[c] == wire_dword(bitwise(poly, buf.data() + 512 * c, 512)), "%s fill %d round of %u chunk %u", name,
              fill, nfr, c);
    }
    for (uint32_t n = 1; n <= 512; n++) {  // every chunk length on the ragged path
      const uint8_t *p = buf.data() + (n * 7u) % 3000u;
      CHECK(ragged_crc(t, p, n) == wire_dword(bitwise(poly, p, n)), "%s fill %d ragged %u", name, fill, n);
    }
  }
}

int main() {
  run(hdfs_crc32c::kPoly, "crc32c", 0xE3069283u);
  run(hdfs_crc32c::kPolyZlib, "crc32", 0xCBF43926u);
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
