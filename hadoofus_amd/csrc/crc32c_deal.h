// The tiled kernels' tune word and the static dealing of schedules 3, 4 and
// 7, written once for the host and the device: tiles_run fills its schedule
// from static_deal(), the speculative batch kernel counts from the same
// function the tiles of each run a workgroup owns, and a host self-test
// (tests/consumer/deal_selftest.cpp) checks both against a walk of every
// workgroup's static tickets.
//
// The dealing.  Tiles come in groups of 2^gshift consecutive tiles.  The
// static phase covers the first phase1() of the tiles when the pool is on
// (all of them when it is off), whole groups only, round-robin over the G
// workgroups; the global pool takes the tiles from p2first on.
//  plain:     workgroup b owns groups b, b + G, b + 2G, ...
//  XCD-major: workgroups are dispatched to the 8 XCDs round-robin (XCD =
//    b % 8), so with the plain dealing the groups an XCD works on at one
//    time are 8 apart; dealing by the virtual id (b % 8) * (G / 8) + b / 8
//    gives each XCD (and its L2) a contiguous run of G / 8 groups per sweep
//    step.
//  XCD-split: XCD x owns the contiguous eighth [x * ngx, (x + 1) * ngx) of
//    the static groups and deals it over its G / 8 workgroups, so the 8 XCDs
//    sweep 8 separate windows (their compute-mode CRC writes land in 8
//    separate regions at any moment); the < 8 leftover groups go to the pool.
// Both XCD forms need G to be a multiple of 8 (else: plain).
// A static ticket is a tile in schedule 3 and a whole group in schedules 4
// and 7 (one wave processes the group's tiles in a row).
#ifndef HADOOFUS_CRC32C_DEAL_H
#define HADOOFUS_CRC32C_DEAL_H

#include <cstdint>

#if defined(__HIPCC__)
#define HDFS_DEAL_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define HDFS_DEAL_HD inline
#endif

#ifndef HDFS_PHASE1_NUM  // A/B builds only (-DHDFS_PHASE1_NUM=n)
#define HDFS_PHASE1_NUM 23
#endif

namespace hdfs_crc32c {

// tune: [7:0] store policy (diagnostic build), [11:8] group shift (log2
// tiles per group; schedule 4: at most 3, one register of CRCs; schedule 7:
// kColShift), [13:12] dealing: 0 plain, 1 XCD-major, 2 XCD-split, [23:16]
// rounds per wave and stream from which the pool is used (0: 32)
HDFS_DEAL_HD uint32_t tune_pack(uint32_t policy, uint32_t gshift, uint32_t xcd, uint32_t pool_min) {
  return (policy & 0xffu) | ((gshift & 15u) << 8) | ((xcd & 3u) << 12) | ((pool_min & 0xffu) << 16);
}
HDFS_DEAL_HD uint32_t tune_policy(uint32_t tune) { return tune & 0xffu; }
HDFS_DEAL_HD uint32_t tune_gshift(uint32_t tune) { return (tune >> 8) & 15u; }
HDFS_DEAL_HD uint32_t tune_xcd(uint32_t tune) { return (tune >> 12) & 3u; }
HDFS_DEAL_HD uint32_t tune_pool_min(uint32_t tune) { return (tune >> 16) & 0xffu; }

constexpr uint32_t kColShift = 2;  // schedule 7: log2 tiles per ticket (32 chunks)
constexpr uint64_t kPhase1Num = HDFS_PHASE1_NUM, kPhase1Den = 25;  // 92 % static

// The static phase's part of x tiles or rounds when the pool is on.
HDFS_DEAL_HD uint64_t phase1(uint64_t x) { return x * kPhase1Num / kPhase1Den; }

// The pool is used from tune_pool_min rounds per wave and stream (lanes =
// waves of the grid x streams per wave); schedules 2 and up.
HDFS_DEAL_HD bool pool_on(uint32_t tune, uint64_t total_rounds, uint32_t lanes) {
  const uint32_t pmin = tune_pool_min(tune);
  return total_rounds >= uint64_t(pmin ? pmin : 32u) * lanes;
}

// Workgroup b's part of the static phase.  T: the tile-count type (uint32_t
// where the caller knows the tiles fit and wants no 64-bit division).
template <class T>
struct Deal {
  bool pool;
  uint32_t gshift;   // log2 tiles per group
  uint32_t kshift;   // log2 static tickets per group: gshift (schedule 3), 0 (4, 7)
  T gfirst;          // the workgroup's first group
  uint32_t gstride;  // groups from one of its groups to the next
  T groups;          // groups it owns: gfirst + i * gstride, i < groups
  T p2first;         // first tile of the pool (== total tiles: no pool tiles)
  HDFS_DEAL_HD uint32_t nk() const { return static_cast<uint32_t>(groups << kshift); }  // its static tickets
};

template <class T>
HDFS_DEAL_HD Deal<T> static_deal(uint32_t tune, int sched, T total_tiles, uint64_t total_rounds, uint32_t lanes,
                                 uint32_t b, uint32_t G) {
  Deal<T> d;
  d.pool = pool_on(tune, total_rounds, lanes);
  const uint32_t gs = tune_gshift(tune);
  d.gshift = sched == 7 ? kColShift : sched == 4 ? (gs < 3u ? gs : 3u) : gs;
  d.kshift = sched == 4 || sched == 7 ? 0u : d.gshift;
  // static phase: whole groups only; the pool takes the rest
  const T ngroups = (d.pool ? static_cast<T>(phase1(total_tiles)) : total_tiles) >> d.gshift;
  const uint32_t xm = tune_xcd(tune);
  if (xm == 2u && (G % 8u) == 0 && ngroups >= T(8) * (G / 8u)) {
    const T ngx = ngroups / 8u;
    const uint32_t G8 = G / 8u, l = b / 8u;
    d.gfirst = (b % 8u) * ngx + l;
    d.gstride = G8;
    d.groups = (ngx - 1 - l) / G8 + 1;
    d.p2first = (ngx * 8u) << d.gshift;
  } else {
    d.gfirst = xm != 0u && (G % 8u) == 0 ? (b % 8u) * (G / 8u) + b / 8u : b;
    d.gstride = G;
    d.groups = ngroups > d.gfirst ? (ngroups - 1 - d.gfirst) / G + 1 : 0;
    d.p2first = ngroups << d.gshift;
  }
  return d;
}

// Static ticket t (below the workgroup's nk) -> global tile.  Schedules 1
// and 2 deal contiguous slices: gfirst is the slice's first tile.
HDFS_DEAL_HD uint64_t static_tile(int sched, uint64_t gfirst, uint32_t gstride, uint32_t gshift, uint32_t t) {
  if (sched == 4 || sched == 7) return (gfirst + uint64_t(t) * gstride) << gshift;
  if (sched == 3) return ((gfirst + uint64_t(t >> gshift) * gstride) << gshift) + (t & ((1u << gshift) - 1u));
  return gfirst + t;
}

// The workgroup's static groups below group x.
template <class T>
HDFS_DEAL_HD T static_groups_below(const Deal<T> &d, T x) {
  if (x <= d.gfirst) return 0;
  const T n = (x - d.gfirst + d.gstride - 1u) / d.gstride;
  return n < d.groups ? n : d.groups;
}

// Static-phase tiles of [t0, t1) the workgroup owns (t0, t1: multiples of
// 2^gshift).  Tiles of the range at or after p2first are not counted.
template <class T>
HDFS_DEAL_HD T static_owned(const Deal<T> &d, T t0, T t1) {
  return (static_groups_below(d, t1 >> d.gshift) - static_groups_below(d, t0 >> d.gshift)) << d.gshift;
}

// A range ending at t1 has tiles of the pool (whose owner is not known in
// advance).
template <class T>
HDFS_DEAL_HD bool reaches_pool(const Deal<T> &d, T t1) {
  return t1 > d.p2first;
}

}  // namespace hdfs_crc32c

#endif
