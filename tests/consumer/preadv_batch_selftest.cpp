// Stand-alone check of the scatter store's arithmetic on the CPU:
// preadv_batch_lookup.h's cursor, piece walk and per-lane decisions, used the
// way unframe_scatter_batch_kernel (preadv_batch_kernels.hip) uses them, against
// a per-byte brute-force model.  Built with -fsanitize=address,undefined by
// tests/test_preadv_batch_cpu.py and run as a program of its own; nothing of
// it is loaded into Python.  No HIP header is needed.
//
// A batch of entries, each with a fragment list of its own (long fragments,
// 16-B multiples, runs of 1- to 15-byte fragments, mixtures), laid in one table
// with fr0 by entry.  One wave's cursor walks the entries in order; inside an
// entry it stores one unit after the other -- rounds of 512 to 4 096 bytes and
// chunks shorter than 512 B -- each cut to [sa, sb) at every alignment, the
// cuts laid end to end over the entry's destination positions.  The stores are
// modelled as the hardware runs them: a range over exactly a piece, an access
// whose offset lies outside dropped.  Checked: every byte of every cut is
// written exactly once, from the right byte of the unit, to the right byte of
// the right fragment; no 16-B store straddles a range's end; nothing outside
// the fragments is written; every table row read lies in the entry's slice;
// the hint is 0 again in every new entry.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "preadv_batch_lookup.h"

using namespace hdfs_preadv_batch;

static long failures;
#define CHECK(c, ...)                      \
  do {                                     \
    if (!(c)) {                            \
      if (failures++ < 20) {               \
        printf("FAIL %s: ", #c);           \
        printf(__VA_ARGS__);               \
        printf("\n");                      \
      }                                    \
    }                                      \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return uint32_t(rng_state >> 33);
}
static uint32_t upto(uint32_t n) { return n ? rnd() % n : 0u; }  // [0, n)

struct Row {
  uint64_t base;  // an address in the model's memory; 0: a sentinel
  uint64_t at;
};

// The `at` column of one slice, with every index checked against the slice.
struct AtOf {
  const Row *t;
  uint32_t nf;
  uint64_t operator[](uint32_t k) const {
    CHECK(k <= nf, "row %u of a slice of %u fragments", k, nf);
    return t[k <= nf ? k : nf].at;
  }
};

// The model's memory: what was written where, how often.
struct Memory {
  std::vector<uint8_t> val;
  std::vector<uint8_t> cnt;
  // a store through the range [a, a + len): dropped when it does not lie inside
  void store(uint64_t a, uint32_t len, uint32_t off, uint32_t size, const uint8_t *src) {
    if (off == kOutside) return;
    if (uint64_t(off) + size > len) {
      // byte stores may wrap below the range or run past it and are dropped; a 16-B one never straddles
      CHECK(size == 1 || off >= len, "a %u-B store at %u straddles the end of a range of %u", size, off, len);
      return;
    }
    for (uint32_t i = 0; i < size; i++) {
      val[a + off + i] = src[i];
      if (cnt[a + off + i] < 255) cnt[a + off + i]++;
    }
  }
};

static uint8_t unit_byte(uint32_t seed, uint32_t i) { return uint8_t((i * 2654435761u + seed * 40503u) >> 11); }

static long n_unseamed, n_seamed, n_small, n_ragged, n_pieces, n_resets;

// One round of n bytes (a multiple of 512, <= 4096) cut to [sa, sb), sa at
// destination position y0 of the cursor's entry: store_scatter's text.
static void store_round_model(Memory &m, const uint32_t *fr0, const Row *ft, uint32_t entry, uint32_t slot, Cursor &c,
                              uint64_t y0, uint32_t n, uint32_t sa, uint32_t sb, uint32_t seed) {
  if (sb == sa) return;  // rule 4
  seek_slot(c, slot);
  const Slice s = slice_of(fr0, entry);
  const Row *t = ft + s.first;
  const AtOf at{t, s.nf};
  const uint32_t k = seek_frag(at, s.nf, y0, c);
  uint8_t reg[64][4][16];
  uint32_t lo[64];
  for (uint32_t lane = 0; lane < 64; lane++) {
    lo[lane] = 64u * (lane & 15u) + 16u * (lane >> 4);
    for (uint32_t j = 0; j < 4; j++)
      for (uint32_t b = 0; b < 16; b++) {
        const uint32_t i = lo[lane] + 1024u * j + b;
        reg[lane][j][b] = i < n ? unit_byte(seed, i) : 0;  // load_round: zeros past the round's chunks
      }
  }
  if (unseamed(at, k, y0, sa, sb, n)) {
    n_unseamed++;
    const uint64_t a = t[k].base + (y0 - t[k].at);
    for (uint32_t lane = 0; lane < 64; lane++)
      for (uint32_t j = 0; j < 4; j++) {
        const uint32_t o = lo[lane] + 1024u * j;  // store_round: the range is the round's chunks
        if (o + 16u <= n) m.store(a, n, o, 16, reg[lane][j]);
      }
    return;
  }
  n_seamed++;
  Walk w{k, sa};
  Piece p;
  uint32_t expect_ps = sa;
  while (next_piece(at, s.nf, y0, sa, sb, w, p)) {
    n_pieces++;
    CHECK(p.ps == expect_ps && p.pe > p.ps && p.pe <= sb && p.k < s.nf, "piece [%u, %u) after %u", p.ps, p.pe,
          expect_ps);
    expect_ps = p.pe;
    if (p.pe - p.ps < 16u) n_small++;
    CHECK(p.foff + (p.pe - p.ps) <= t[p.k + 1].at - t[p.k].at, "a piece leaves its fragment");
    const uint64_t a = t[p.k].base + p.foff;
    const uint32_t len = p.pe - p.ps;
    uint32_t q0 = 0, q1 = 0;
    const bool he = head_edge(p.ps, p.pe, q0), te = tail_edge(p.ps, p.pe, q1);
    for (uint32_t lane = 0; lane < 64; lane++) {
      for (uint32_t j = 0; j < 4; j++) m.store(a, len, whole_at(lo[lane] + 1024u * j, p.ps, p.pe), 16, reg[lane][j]);
      for (int edge = 0; edge < 2; edge++) {
        if (!(edge ? te : he)) continue;
        const uint32_t o = 16u * (edge ? q1 : q0), kq = o >> 10;
        const bool mine = lo[lane] == (o & 1023u);
        for (uint32_t b = 0; b < 16; b++)
          m.store(a, len, mine ? byte_at(o + b, p.ps, p.pe) : kOutside, 1, &reg[lane][kq][b]);
      }
    }
  }
  CHECK(expect_ps == sb, "the walk ended at %u of [%u, %u)", expect_ps, sa, sb);
}

// The chunk of n < 512 bytes cut to [sa, sb): verify_ragged's stores.
static void store_ragged_model(Memory &m, const uint32_t *fr0, const Row *ft, uint32_t entry, uint32_t slot,
                               Cursor &c, uint64_t y0, uint32_t n, uint32_t sa, uint32_t sb, uint32_t seed) {
  if (sb == sa) return;
  n_ragged++;
  seek_slot(c, slot);
  const Slice s = slice_of(fr0, entry);
  const Row *t = ft + s.first;
  const AtOf at{t, s.nf};
  const uint32_t pad = 512u - n;
  Walk w{seek_frag(at, s.nf, y0, c), sa};
  Piece p;
  uint32_t expect_ps = sa;
  while (next_piece(at, s.nf, y0, sa, sb, w, p)) {
    n_pieces++;
    CHECK(p.ps == expect_ps && p.pe > p.ps && p.pe <= sb, "ragged piece [%u, %u) after %u", p.ps, p.pe, expect_ps);
    expect_ps = p.pe;
    if (p.pe - p.ps < 16u) n_small++;
    const uint64_t a = t[p.k].base + p.foff;
    const uint32_t skip = pad + p.ps;
    for (uint32_t lane = 0; lane < 64; lane++)
      for (uint32_t j = 0; j < 8; j++) {
        const uint32_t f = 8u * lane + j;
        const uint8_t b = f >= pad ? unit_byte(seed, f - pad) : 0;
        m.store(a, p.pe - p.ps, f - skip, 1, &b);  // the offset wraps below the piece: outside the range
      }
  }
  CHECK(expect_ps == sb, "the ragged walk ended at %u of [%u, %u)", expect_ps, sa, sb);
}

// Fragment lengths of an entry of `total` bytes, in one of four styles.
static std::vector<uint32_t> fragments(uint64_t total, uint32_t style) {
  std::vector<uint32_t> v;
  uint64_t left = total;
  uint32_t run = 0;  // tiny fragments still to come in the current run
  while (left) {
    uint32_t n;
    if (style == 0) {
      n = 3000u + upto(30000u);
    } else if (style == 1) {
      n = 16u * (1u + upto(40u));
    } else if (style == 2) {
      n = 1u + upto(15u);
    } else {
      if (!run && upto(4u) == 0u) run = 1u + upto(40u);
      if (run) {
        run--;
        n = 1u + upto(15u);
      } else {
        n = upto(3u) == 0u ? 4096u * (1u + upto(3u)) : 1u + upto(5000u);
      }
    }
    if (n > left) n = uint32_t(left);
    v.push_back(n);
    left -= n;
  }
  return v;
}

int main() {
  const uint32_t kGap = 40;  // guard bytes around every fragment in the model's memory
  for (uint32_t trial = 0; trial < 60; trial++) {
    const uint32_t n = 2u + upto(5u);
    // the entries' cuts first: their totals are the read lengths
    struct Cut {
      uint32_t unit, sa, sb;
      bool ragged;
    };
    std::vector<std::vector<Cut>> cuts(n);
    std::vector<uint64_t> total(n, 0);
    std::vector<uint32_t> style(n);
    for (uint32_t e = 0; e < n; e++) {
      style[e] = (trial + e) % 4u;
      const uint32_t units = style[e] == 2u ? 3u + upto(4u) : 20u + upto(40u);
      for (uint32_t i = 0; i < units; i++) {
        Cut c;
        c.ragged = upto(5u) == 0u;
        c.unit = c.ragged ? 1u + upto(511u) : 512u * (1u + upto(8u));
        const uint32_t how = upto(8u);
        if (how < 3u) {  // the whole unit
          c.sa = 0;
          c.sb = c.unit;
        } else if (how == 3u) {  // nothing of it
          c.sa = c.sb = upto(c.unit + 1u);
        } else {  // both ends anywhere
          c.sa = upto(c.unit + 1u);
          c.sb = c.sa + upto(c.unit - c.sa + 1u);
        }
        cuts[e].push_back(c);
        total[e] += c.sb - c.sa;
      }
      if (!total[e]) {
        cuts[e].push_back(Cut{512, 0, 512, false});
        total[e] = 512;
      }
    }
    // the tables: an entry's fragments, then its sentinel; room behind the read in a last fragment now and then
    std::vector<Row> ft;
    std::vector<uint32_t> fr0;
    struct Place {
      uint32_t entry, k, len;
    };
    std::vector<Place> places;
    for (uint32_t e = 0; e < n; e++) {
      fr0.push_back(uint32_t(ft.size()));
      const uint64_t cap = total[e] + (upto(2u) ? upto(100u) : 0u);
      uint64_t at = 0;
      uint32_t k = 0;
      for (uint32_t len : fragments(cap, style[e])) {
        ft.push_back(Row{0, at});
        places.push_back(Place{e, k++, len});
        at += len;
      }
      ft.push_back(Row{0, at});
    }
    fr0.push_back(uint32_t(ft.size()));
    // bases in shuffled order, guards between
    for (size_t i = places.size(); i > 1; i--) std::swap(places[i - 1], places[upto(uint32_t(i))]);
    uint64_t addr = kGap;
    for (const Place &p : places) {
      ft[fr0[p.entry] + p.k].base = addr + upto(16u);
      addr = ft[fr0[p.entry] + p.k].base + p.len + kGap;
    }
    Memory m;
    m.val.assign(addr + 64, 0);
    m.cnt.assign(addr + 64, 0);
    std::vector<uint8_t> want(addr + 64, 0), wcnt(addr + 64, 0);
    // one wave's walk: slots in order (here slot = entry; an entry now and then left out, as an irregular one is)
    Cursor c;
    for (uint32_t e = 0; e < n; e++) {
      const Slice s = slice_of(fr0.data(), e);
      const Row *t = ft.data() + s.first;
      uint64_t y = 0;
      bool first = true;
      for (size_t i = 0; i < cuts[e].size(); i++) {
        const Cut &u = cuts[e][i];
        const uint32_t seed = trial * 1000u + e * 100u + uint32_t(i);
        // brute force: byte by byte, a linear scan for the fragment
        for (uint32_t b = u.sa; b < u.sb; b++) {
          const uint64_t pos = y + (b - u.sa);
          uint32_t k = 0;
          while (k < s.nf && t[k + 1].at <= pos) k++;
          const uint64_t a = t[k].base + (pos - t[k].at);
          want[a] = unit_byte(seed, b);
          wcnt[a]++;
        }
        const uint32_t kf_before = c.kf, slot_before = c.slot;
        if (u.ragged)
          store_ragged_model(m, fr0.data(), ft.data(), e, e, c, y, u.unit, u.sa, u.sb, seed);
        else
          store_round_model(m, fr0.data(), ft.data(), e, e, c, y, u.unit, u.sa, u.sb, seed);
        if (u.sb > u.sa) {
          if (first && slot_before != e) n_resets++;
          if (first) CHECK(c.slot == e, "the cursor's slot after entry %u's first store", e);
          if (!first) CHECK(c.kf >= kf_before, "the hint fell inside an entry");
          first = false;
          uint32_t k = 0;
          while (k < s.nf && t[k + 1].at <= y) k++;
          CHECK(c.kf == k, "hint %u, fragment %u", c.kf, k);
        } else {
          CHECK(c.kf == kf_before && c.slot == slot_before, "an empty cut moved the cursor");
        }
        y += u.sb - u.sa;
      }
    }
    long bad = 0;
    for (size_t a = 0; a < want.size(); a++)
      if (m.cnt[a] != wcnt[a] || m.val[a] != want[a]) bad++;
    CHECK(bad == 0, "trial %u: %ld bytes written wrongly, not once, or outside the cuts", trial, bad);
  }
  // the hint's reset, on its own: a slice of one fragment behind one of many
  {
    const uint32_t fr0[3] = {0, 6, 8};
    const uint64_t at[8] = {0, 1, 2, 3, 4, 5, 0, 9};
    Cursor c;
    seek_slot(c, 0);
    Slice s = slice_of(fr0, 0u);
    CHECK(s.first == 0 && s.nf == 5, "slice 0");
    CHECK(seek_frag(at, s.nf, 4, c) == 4 && c.kf == 4, "fragment 4");
    seek_slot(c, 0);
    CHECK(c.kf == 4, "the hint stays inside an entry");
    seek_slot(c, 1);
    CHECK(c.kf == 0 && c.slot == 1, "the hint is 0 again in the next entry");
    s = slice_of(fr0, 1u);
    CHECK(s.first == 6 && s.nf == 1 && seek_frag(at + s.first, s.nf, 8, c) == 0, "slice 1");
  }
  printf("%ld unseamed rounds, %ld seamed rounds, %ld pieces below 16 B, %ld ragged chunks, %ld pieces, %ld resets\n",
         n_unseamed, n_seamed, n_small, n_ragged, n_pieces, n_resets);
  printf("%ld failures\n", failures);
  return failures != 0;
}
