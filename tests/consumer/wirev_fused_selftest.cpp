// Stand-alone check of the fused gather library's host-and-device code on the
// CPU (wirev_fused_lookup.h): frag_of, the function frame_fused_gather_kernel
// runs on the scalar unit, against a linear scan of the same offsets, and
// count_packet, the routine behind hdfs_wirev_fused_layout's rounds,
// seamed_rounds, seamed_ragged and max_frags_per_round, against a brute-force
// model that asks for every byte which fragment holds it.  Built with
// -fsanitize=address,undefined by tests/test_wirev_fused_cpu.py and run as a
// child process; nothing of it is loaded into Python.  The `at` array is
// allocated at exactly nf + 1 words, so a read outside it is the sanitizer's
// to report.
//
// frag_of: tables of 1, 2, 3, 17 and 65 536 fragments, with lengths all ones,
// all large, alternating 1 / 100 000, and one huge fragment among ones (first,
// middle, last).  For the first and the last byte of every fragment (and the
// bytes next to them):
//   * up to 17 fragments: every hint <= the answer;
//   * 65 536 fragments: the hints at distance 0 .. kFragHops + 1 below the
//     answer (the hops end before, exactly at and one past the hop bound), and
//     also hint 0, half the answer and every power of two below the answer,
//     which send the lookup far into its binary search.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wirev_fused_lookup.h"

using hdfs_wirev_fused::count_packet;
using hdfs_wirev_fused::frag_of;
using hdfs_wirev_fused::kFragHops;
using hdfs_wirev_fused::RoundCounts;

static int failures = 0;
static unsigned long long checks = 0;

static uint64_t *table(const std::vector<uint64_t> &lens) {
  const size_t nf = lens.size();
  uint64_t *at = new uint64_t[nf + 1];  // exactly nf + 1 words on the heap
  uint64_t sum = 0;
  for (size_t k = 0; k < nf; k++) {
    at[k] = sum;
    sum += lens[k];
  }
  at[nf] = sum;
  return at;
}

static void check(const uint64_t *at, uint32_t nf, uint64_t pos, uint32_t hint, uint32_t want, const char *name) {
  checks++;
  const uint32_t got = frag_of(at, nf, pos, hint);
  if (got != want) {
    failures++;
    if (failures < 20)
      std::printf("FAIL %s: nf %u pos %llu hint %u: got %u, want %u\n", name, nf, (unsigned long long)pos, hint, got,
                  want);
  }
}

static void lookups(const char *name, const std::vector<uint64_t> &lens) {
  const uint32_t nf = uint32_t(lens.size());
  uint64_t *at = table(lens);
  const bool all_hints = nf <= 17u;
  for (uint32_t k = 0; k < nf; k++) {  // the linear scan: k is the answer of every byte of [at[k], at[k + 1])
    const uint64_t first = at[k], last = at[k + 1] - 1u;
    uint64_t probes[5] = {first, last, first + 1u, last - 1u, first + (last - first) / 2u};
    for (const uint64_t pos : probes) {
      if (pos < first || pos > last) continue;
      if (all_hints) {
        for (uint32_t h = 0; h <= k; h++) check(at, nf, pos, h, k, name);
        continue;
      }
      for (uint32_t d = 0; d <= kFragHops + 1u && d <= k; d++) check(at, nf, pos, k - d, k, name);
      check(at, nf, pos, 0u, k, name);
      check(at, nf, pos, k / 2u, k, name);
      for (uint32_t d = 1; d <= k; d <<= 1) check(at, nf, pos, k - d, k, name);
    }
  }
  delete[] at;
}

// ---- the rounds of a write, counted twice ----------------------------------------------
// Brute force: the fragment of every byte by linear scan, a round's fragments
// the distinct ones among its bytes.  Packets as packet_at cuts them: a short
// first packet of n0 bytes, then 64 KiB packets.
static void rounds(const char *name, const std::vector<uint64_t> &lens, uint32_t n0) {
  const uint32_t nf = uint32_t(lens.size());
  uint64_t *at = table(lens);
  const uint64_t len = at[nf];
  std::vector<uint32_t> owner(len);
  for (uint32_t k = 0; k < nf; k++)
    for (uint64_t p = at[k]; p < at[k + 1]; p++) owner[p] = k;
  auto distinct = [&](uint64_t a, uint64_t e) { return owner[e - 1] - owner[a] + 1u; };  // owners rise along the write
  RoundCounts got, want;
  uint32_t hint = 0;
  uint64_t a = 0;
  while (a < len) {
    const uint64_t left = len - a;
    const uint32_t dlen = uint32_t(a == 0 && n0 ? (n0 < left ? n0 : left) : (left < 65536u ? left : 65536u));
    count_packet(at, nf, a, dlen, hint, got);
    const uint32_t full = dlen / 512u * 512u;
    for (uint32_t r = 0; r < full; r += 4096u) {
      const uint32_t e = full - r < 4096u ? full : r + 4096u;
      const uint32_t n = distinct(a + r, a + e);
      want.rounds++;
      want.seamed_rounds += n > 1u;
      if (n > want.max_frags_per_round) want.max_frags_per_round = n;
    }
    if (dlen % 512u) want.seamed_ragged += distinct(a + full, a + dlen) > 1u;
    a += dlen;
  }
  checks++;
  if (got.rounds != want.rounds || got.seamed_rounds != want.seamed_rounds || got.seamed_ragged != want.seamed_ragged ||
      got.max_frags_per_round != want.max_frags_per_round) {
    failures++;
    std::printf("FAIL rounds of %s, n0 %u: got %llu/%llu/%llu/%u, want %llu/%llu/%llu/%u\n", name, n0,
                (unsigned long long)got.rounds, (unsigned long long)got.seamed_rounds,
                (unsigned long long)got.seamed_ragged, got.max_frags_per_round, (unsigned long long)want.rounds,
                (unsigned long long)want.seamed_rounds, (unsigned long long)want.seamed_ragged,
                want.max_frags_per_round);
  }
  delete[] at;
}

int main() {
  static const uint32_t sizes[] = {1, 2, 3, 17, 65536};
  for (const uint32_t nf : sizes) {
    const uint64_t large = nf > 17u ? 70000u : 3u << 20, huge = uint64_t(1) << 39;
    std::vector<uint64_t> c(nf);
    for (uint32_t k = 0; k < nf; k++) c[k] = 1u;
    lookups("all ones", c);
    for (uint32_t k = 0; k < nf; k++) c[k] = large;
    lookups("all large", c);
    for (uint32_t k = 0; k < nf; k++) c[k] = (k & 1u) ? 100000u : 1u;
    lookups("alternating 1 / 100000", c);
    for (uint32_t at : {0u, nf / 2u, nf - 1u}) {
      for (uint32_t k = 0; k < nf; k++) c[k] = k == at ? huge : 1u;
      lookups("one huge fragment among ones", c);
    }
  }
  // the rounds: a few hundred KiB in fragments of every kind, aligned and with a short first packet
  struct Shape {
    const char *name;
    std::vector<uint64_t> lens;
  };
  std::vector<Shape> shapes;
  shapes.push_back({"one fragment", {3 * 65536 + 700}});
  shapes.push_back({"two fragments", {287 + 4096 + 1, 2 * 65536}});
  shapes.push_back({"ones", std::vector<uint64_t>(70000, 1)});
  shapes.push_back({"4097s", std::vector<uint64_t>(50, 4097)});
  shapes.push_back({"4096s", std::vector<uint64_t>(50, 4096)});
  shapes.push_back({"512s", std::vector<uint64_t>(300, 512)});
  shapes.push_back({"511s", std::vector<uint64_t>(300, 511)});
  {
    std::vector<uint64_t> v;
    uint64_t x = 88172645463325252ull;  // xorshift: lengths 1 .. 9000
    for (int k = 0; k < 120; k++) {
      x ^= x << 13;
      x ^= x >> 7;
      x ^= x << 17;
      v.push_back(1u + x % ((k % 3) ? 9000u : 40u));
    }
    shapes.push_back({"random", v});
  }
  for (const Shape &s : shapes)
    for (const uint32_t n0 : {0u, 287u, 1u, 511u}) rounds(s.name, s.lens, n0);
  std::printf("%llu checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
