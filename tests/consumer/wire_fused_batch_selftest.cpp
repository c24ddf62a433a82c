// Stand-alone check of the fused batch library's lookup on the CPU:
// write_of (wire_fused_batch_lookup.h), the function frame_fused_batch_kernel
// runs on the scalar unit, against a linear scan of the same prefix array.
// Built with -fsanitize=address,undefined by tests/test_wire_fused_batch_cpu.py
// and run as a child process; nothing of it is loaded into Python.  The prefix
// array is allocated at exactly nw + 1 words, so a read outside it is the
// sanitizer's to report.
//
// Tables of 1, 2, 3, 17 and 65 536 entries, with packet counts all ones, all
// large, alternating 1 / 1000, and one huge entry among ones.  For every g of
// every table (so g = pk0[k] and g = pk0[k + 1] - 1 of every k among them):
//   * up to 17 entries: every hint <= the answer;
//   * 65 536 entries: the hints at distance 0 .. kLookupHops + 1 below the
//     answer (the hops end before, exactly at and one past the hop bound), and
//     at the first, middle and last g of every entry also hint 0, half the
//     answer and every power of two below the answer, which send the lookup
//     far into its binary search.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wire_fused_batch_lookup.h"

using hdfs_wire_fused::kLookupHops;
using hdfs_wire_fused::write_of;

static int failures = 0;
static unsigned long long checks = 0;

static void check(const uint32_t *pk0, uint32_t nw, uint32_t g, uint32_t hint, uint32_t want, const char *name) {
  checks++;
  const uint32_t got = write_of(pk0, nw, g, hint);
  if (got != want) {
    failures++;
    if (failures < 20) std::printf("FAIL %s: nw %u g %u hint %u: got %u, want %u\n", name, nw, g, hint, got, want);
  }
}

static void run(const char *name, const std::vector<uint32_t> &counts) {
  const uint32_t nw = uint32_t(counts.size());
  // exactly nw + 1 words on the heap
  uint32_t *pk0 = new uint32_t[nw + 1];
  uint64_t sum = 0;
  for (uint32_t k = 0; k < nw; k++) {
    pk0[k] = uint32_t(sum);
    sum += counts[k];
  }
  pk0[nw] = uint32_t(sum);
  if (sum > 0x7FFFFFFFull / 4u) {
    std::printf("FAIL %s: the table has more packets than a batch may\n", name);
    failures++;
  }
  const bool all_hints = nw <= 17u;
  uint32_t k = 0;  // the linear scan: the answer only grows with g
  for (uint32_t g = 0; g < pk0[nw]; g++) {
    while (g >= pk0[k + 1]) k++;
    if (all_hints) {
      for (uint32_t h = 0; h <= k; h++) check(pk0, nw, g, h, k, name);
      continue;
    }
    for (uint32_t d = 0; d <= kLookupHops + 1u && d <= k; d++) check(pk0, nw, g, k - d, k, name);
    const uint32_t first = pk0[k], last = pk0[k + 1] - 1u, mid = first + (last - first) / 2u;
    if (g == first || g == last || g == mid) {
      check(pk0, nw, g, 0u, k, name);
      check(pk0, nw, g, k / 2u, k, name);
      for (uint32_t d = 1; d <= k; d <<= 1) check(pk0, nw, g, k - d, k, name);
    }
  }
  delete[] pk0;
}

int main() {
  static const uint32_t sizes[] = {1, 2, 3, 17, 65536};
  for (const uint32_t nw : sizes) {
    const uint32_t large = nw > 17u ? 100u : 2049u, huge = nw > 17u ? (1u << 20) : 100000u;
    std::vector<uint32_t> c(nw);
    for (uint32_t k = 0; k < nw; k++) c[k] = 1u;
    run("all ones", c);
    for (uint32_t k = 0; k < nw; k++) c[k] = large;
    run("all large", c);
    for (uint32_t k = 0; k < nw; k++) c[k] = (k & 1u) ? 1000u : 1u;
    run("alternating 1 / 1000", c);
    if (nw <= 17u) {
      for (uint32_t k = 0; k < nw; k++) c[k] = (k & 1u) ? 1u : 1000u;
      run("alternating 1000 / 1", c);
    }
    for (uint32_t at : {0u, nw / 2u, nw - 1u}) {
      for (uint32_t k = 0; k < nw; k++) c[k] = k == at ? huge : 1u;
      run("one huge entry among ones", c);
    }
  }
  std::printf("%llu checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
