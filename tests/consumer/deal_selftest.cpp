// Self-test of hadoofus_amd/csrc/crc32c_deal.h on the host (built with
// ASan/UBSan by tests/test_deal.py): the static dealing of the tiled kernels
// and the per-run tile counts of the speculative batch kernel, which both
// come from static_deal(), against a brute-force walk of every workgroup's
// static tickets through static_tile().
//
// Launches: a batch of `runs` equal runs of `ppr` packets of `tpp` tiles of
// `rpt` rounds, on G workgroups of 16 waves with one stream each.  Every
// dealing (G x group shift x XCD mode x pool minimum, 288) meets kShapes
// launch shapes taken from the shape grid (runs 2..16 x tiles per packet
// 1, 2, 16 x packets per run 1..40 x rounds per tile 1, 8) at a stride
// coprime to its size, so every value of every shape parameter occurs; the
// cases whose tiles per run are whole groups are kept (a few thousand).
//  1. the static tickets of all workgroups cover [0, p2first) exactly once
//     and nothing from p2first on; p2first <= total tiles, whole groups;
//  2. schedule 3: static_owned() of each run without pool tiles equals the
//     workgroup's static tickets in the run, and over all runs adds up to nk;
//  3. the 32-bit and 64-bit instantiations agree on every field and count;
//  4. property 1 with the group-sized tickets of schedules 4 (group shift
//     clamped to 3) and 7 (kColShift);
//  5. the tune word round-trips every field at its extremes.
// Prints "N failures".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "crc32c_deal.h"

using namespace hdfs_crc32c;

static int g_fail = 0;
static char g_case[160] = "";
#define CHECK(c)                                                                                       \
  do {                                                                                                  \
    if (!(c)) {                                                                                         \
      if (g_fail < 20) std::printf("FAIL %s:%d: %s [%s]\n", __FILE__, __LINE__, #c, g_case);           \
      g_fail++;                                                                                         \
    }                                                                                                   \
  } while (0)

struct Seen {
  unsigned cases = 0, pool = 0, split = 0, major = 0, pool_runs = 0, idle = 0;
};

static void check_launch(uint32_t tune, int sched, uint32_t G, uint32_t runs, uint32_t per_t, uint32_t rpt,
                         Seen &seen) {
  const uint64_t total = uint64_t(runs) * per_t, rounds = total * rpt;
  const uint32_t lanes = G * 16u;
  const uint32_t gs = tune_gshift(tune), want_gshift = sched == 7 ? kColShift : sched == 4 ? (gs < 3u ? gs : 3u) : gs;
  std::vector<uint8_t> cover(total, 0);
  std::vector<uint32_t> in_run(runs);
  uint64_t p2first = 0;
  for (uint32_t b = 0; b < G; b++) {
    const Deal<uint64_t> d = static_deal<uint64_t>(tune, sched, total, rounds, lanes, b, G);
    const Deal<uint32_t> e = static_deal<uint32_t>(tune, sched, uint32_t(total), rounds, lanes, b, G);
    // 3: one dealing at both widths
    CHECK(d.pool == e.pool && d.gshift == e.gshift && d.kshift == e.kshift && d.gfirst == e.gfirst &&
          d.gstride == e.gstride && d.groups == e.groups && d.p2first == e.p2first && d.nk() == e.nk());
    CHECK(d.gshift == want_gshift);
    CHECK(d.pool == pool_on(tune, rounds, lanes));
    CHECK(d.nk() == (sched == 3 ? d.groups << d.gshift : d.groups));
    const uint64_t gsize = 1ull << d.gshift;
    if (b == 0) {
      p2first = d.p2first;
      CHECK(p2first <= total && p2first % gsize == 0);
      CHECK(d.pool || total - p2first < (tune_xcd(tune) == 2u ? 8u : 1u) * gsize);
      seen.pool += d.pool;
      seen.split += d.gstride != G;
    }
    seen.major += b == 1 && d.gstride == G && d.gfirst != 1;
    CHECK(d.p2first == p2first);
    seen.idle += d.groups == 0;
    // 1 / 4: the walk of the workgroup's static tickets
    for (uint32_t &c : in_run) c = 0;
    for (uint32_t t = 0; t < d.nk(); t++) {
      const uint64_t g = static_tile(sched, d.gfirst, d.gstride, d.gshift, t);
      const uint64_t n = sched == 3 ? 1u : gsize;
      CHECK(g + n <= p2first);
      if (g + n > total) continue;
      for (uint64_t i = 0; i < n; i++) cover[g + i]++;
      in_run[g / per_t]++;
    }
    if (sched != 3) continue;
    // 2: the counts of the batch kernel's prologue
    uint64_t sum = 0, sum32 = 0;
    for (uint32_t r = 0; r < runs; r++) {
      const uint64_t t0 = uint64_t(r) * per_t, t1 = t0 + per_t;
      const uint64_t own = static_owned(d, t0, t1);
      const uint32_t own32 = static_owned(e, uint32_t(t0), uint32_t(t1));
      CHECK(own == own32 && reaches_pool(d, t1) == reaches_pool(e, uint32_t(t1)));
      CHECK(reaches_pool(d, t1) == (t1 > p2first));
      if (!reaches_pool(d, t1)) CHECK(own == in_run[r]);
      else if (b == 0) seen.pool_runs++;
      sum += own;
      sum32 += own32;
    }
    CHECK(sum == d.nk() && sum32 == d.nk());
  }
  for (uint64_t g = 0; g < total; g++) CHECK(cover[g] == (g < p2first ? 1 : 0));
  seen.cases++;
}

int main() {
  // 5: the tune word
  for (uint32_t i = 0; i < 16; i++) {
    const uint32_t p = i & 1 ? 0xffu : 0u, g = i & 2 ? 15u : 0u, x = i & 4 ? 3u : 0u, m = i & 8 ? 0xffu : 0u;
    const uint32_t t = tune_pack(p, g, x, m);
    std::snprintf(g_case, sizeof g_case, "tune %u %u %u %u", p, g, x, m);
    CHECK(t == (p | (g << 8) | (x << 12) | (m << 16)));
    CHECK(tune_policy(t) == p && tune_gshift(t) == g && tune_xcd(t) == x && tune_pool_min(t) == m);
  }
  CHECK(tune_pack(0x1ffu, 16u, 4u, 0x100u) == 0xffu);  // a field never spills into its neighbour

  const uint32_t Gs[] = {1, 2, 7, 8, 16, 24, 250, 256}, gshifts[] = {0, 1, 3, 4}, pmins[] = {0, 1, 4};
  const uint32_t tpps[] = {1, 2, 16}, rpts[] = {1, 8};
  constexpr uint32_t kShapeGrid = 15 * 3 * 40 * 2, kShapes = 13, kStep = 277;  // 277: prime, not a factor of 3600
  Seen seen3, seen4, seen7;
  uint32_t k = 0;
  for (uint32_t G : Gs)
    for (uint32_t gshift : gshifts)
      for (uint32_t xm = 0; xm < 3; xm++)
        for (uint32_t pmin : pmins)
          for (uint32_t j = 0; j < kShapes; j++, k = (k + kStep) % kShapeGrid) {
            const uint32_t runs = 2 + k % 15, tpp = tpps[k / 15 % 3], ppr = 1 + k / 45 % 40, rpt = rpts[k / 1800];
            const uint32_t per_t = tpp * ppr;
            if (per_t & ((1u << gshift) - 1u)) continue;  // per-run completion needs whole groups per run
            const uint32_t tune = tune_pack(0, gshift, xm, pmin);
            std::snprintf(g_case, sizeof g_case, "G %u gshift %u xcd %u pmin %u runs %u tpp %u ppr %u rpt %u", G,
                          gshift, xm, pmin, runs, tpp, ppr, rpt);
            check_launch(tune, 3, G, runs, per_t, rpt, seen3);
            check_launch(tune, 4, G, runs, per_t, rpt, seen4);
            check_launch(tune, 7, G, runs, per_t, rpt, seen7);
          }
  g_case[0] = 0;
  // the sweep met every form of the dealing
  CHECK(seen3.cases >= 2000 && seen3.cases == seen4.cases && seen3.cases == seen7.cases);
  CHECK(seen3.pool > 100 && seen3.cases - seen3.pool > 100 && seen3.split > 100 && seen3.major > 100);
  CHECK(seen3.pool_runs > 100 && seen3.idle > 100);
  std::printf("%u cases per schedule: pool on %u, XCD-split %u, XCD-major %u, runs with pool tiles %u, "
              "idle workgroups %u\n",
              seen3.cases, seen3.pool, seen3.split, seen3.major, seen3.pool_runs, seen3.idle);
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
