// Stand-alone check of the fused gather batch library's host-and-device index
// logic on the CPU (wirev_fused_batch_lookup.h: seek_write, slice_of,
// seek_frag and the cursor copy that the ragged chunk gets) against a
// brute-force model that knows every packet's write and finds every byte's
// fragment by a linear scan of that write's own offsets.  Built with
// -fsanitize=address,undefined by tests/test_wirev_fused_batch_cpu.py and run
// as a child process; nothing of it is loaded into Python.
//
// The tables are those of wirev_fused_batch_internal.h, each allocated on the
// heap at exactly its size (a read past a table is the sanitizer's to report),
// and the fragment table is read through an accessor that knows the current
// slice's bounds, so a read inside the table but outside the slice -- a stale
// hint's -- is reported too.
//
// The walk is the kernel's: for G in {1, 3, 7, 256}, workgroup b takes global
// packets g = b, b + G, ...; each of the 16 waves carries its own cursor; the
// next packet's lookups run ahead of the current packet's ragged chunk, which
// wave 0 looks up with the cursor copied when the current packet's lookups
// were done.  Per step it checks: the write found; that a g at or past the
// total and a round without a full chunk look nothing up and leave the cursor
// alone; the slice; that the hint handed to frag_of is no later than the
// answer; the fragment found, for the round and for the ragged chunk.
//
// It also counts every batch's rounds the way hdfs_wirev_fused_batch_layout
// does (count_packet per write, the hint from 0 for each, sums and the
// maximum) against the model's own count.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "wirev_fused_batch_lookup.h"

using hdfs_wirev_fused::count_packet;
using hdfs_wirev_fused::frag_of;
using hdfs_wirev_fused::RoundCounts;
using hdfs_wirev_fused_batch::Cursor;
using hdfs_wirev_fused_batch::seek_frag;
using hdfs_wirev_fused_batch::seek_write;
using hdfs_wirev_fused_batch::Slice;
using hdfs_wirev_fused_batch::slice_of;

static int failures = 0;
static unsigned long long checks = 0;

#define CHECK(cond, ...)                        \
  do {                                          \
    checks++;                                   \
    if (!(cond)) {                              \
      if (failures++ < 20) {                    \
        std::printf("FAIL %s: ", #cond);        \
        std::printf(__VA_ARGS__);               \
        std::printf("\n");                      \
      }                                         \
    }                                           \
  } while (0)

// ---- the model --------------------------------------------------------------------------
struct ModelWrite {
  std::vector<uint64_t> at;  // nf + 1: where each non-empty fragment starts, then the length
  uint32_t n0 = 0;           // bytes of the short first packet the block offset asks for (cut to the length)
  bool finish = false;
  uint64_t len() const { return at.back(); }
  uint32_t nf() const { return uint32_t(at.size() - 1); }
  uint32_t head() const { return uint32_t(n0 < len() ? n0 : len()); }
  uint64_t npk() const {
    const uint64_t body = len() - head();
    return (head() ? 1u : 0u) + (body + 65535u) / 65536u + (finish ? 1u : 0u);
  }
  // packet i: its first byte in the write and its data bytes
  void packet(uint64_t i, uint64_t &a, uint32_t &dlen) const {
    const uint64_t k0 = head() ? 1u : 0u;
    if (i < k0) {
      a = 0, dlen = head();
      return;
    }
    const uint64_t body = len() - head(), off = (i - k0) * 65536u < body ? (i - k0) * 65536u : body;
    a = head() + off;
    dlen = uint32_t(body - off < 65536u ? body - off : 65536u);
  }
  uint32_t frag(uint64_t pos) const {  // linear scan
    uint32_t k = 0;
    while (!(at[k] <= pos && pos < at[k + 1])) k++;
    return k;
  }
  uint32_t under(uint64_t a, uint64_t e) const { return frag(e - 1) - frag(a) + 1u; }
};

static ModelWrite mw(const std::vector<uint64_t> &lens, uint32_t n0, bool finish) {
  ModelWrite w;
  uint64_t sum = 0;
  for (const uint64_t l : lens) {
    if (l) w.at.push_back(sum);
    sum += l;
  }
  w.at.push_back(sum);
  w.n0 = n0;
  w.finish = finish;
  return w;
}

// ---- the tables, each at exactly its size ---------------------------------------------------
struct Tables {
  std::vector<const ModelWrite *> w;  // the writes that have packets, in batch order
  uint64_t *at = nullptr;             // the fragment table's `at` column
  uint32_t *pk0 = nullptr, *fr0 = nullptr;
  uint32_t nw = 0, total = 0, nfe = 0;
  ~Tables() {
    delete[] at;
    delete[] pk0;
    delete[] fr0;
  }
};

static void build(const std::vector<ModelWrite> &batch, Tables &t) {
  for (const ModelWrite &w : batch)
    if (w.npk()) {
      t.w.push_back(&w);
      t.nfe += w.nf() + 1u;
    }
  t.nw = uint32_t(t.w.size());
  t.at = new uint64_t[t.nfe];
  t.pk0 = new uint32_t[t.nw + 1];
  t.fr0 = new uint32_t[t.nw + 1];
  uint32_t f = 0;
  uint64_t pk = 0;
  for (uint32_t k = 0; k < t.nw; k++) {
    t.pk0[k] = uint32_t(pk);
    t.fr0[k] = f;
    for (const uint64_t a : t.w[k]->at) t.at[f++] = a;
    pk += t.w[k]->npk();
  }
  t.pk0[t.nw] = t.total = uint32_t(pk);
  t.fr0[t.nw] = f;
}

// The `at` column of one slice; an index outside [0, nf] is another write's entry.
struct SliceAt {
  const uint64_t *p;
  uint32_t nf;
  const char *name;
  uint64_t operator[](uint32_t k) const {
    CHECK(k <= nf, "%s: entry %u of a slice of %u fragments", name, k, nf);
    return k <= nf ? p[k] : ~uint64_t(0);
  }
};

// ---- the walk ---------------------------------------------------------------------------
// limit: the walk ends at global packet `limit` (the whole batch: its total);
// every: 0 walks every workgroup, otherwise only those whose index it divides
// and the last one.
static void walk(const char *name, const Tables &t, uint32_t G, uint32_t limit, uint32_t every) {
  for (uint32_t b = 0; b < G; b++) {
    if (every && b % every && b + 1u != G) continue;
    Cursor c[16], kc[16];
    uint32_t model_k = 0;  // the model's write of the packet looked up last: a scan that only moves forward
    // one wave's lookups of global packet g, as load_unit_at does them
    auto unit = [&](uint32_t g, uint32_t v) {
      const Cursor before = c[v];
      const bool in = seek_write(t.pk0, t.nw, t.total, g, c[v]);
      CHECK(in == (g < t.total), "%s: G %u g %u", name, G, g);
      if (!in) {
        CHECK(c[v].kw == before.kw && c[v].kf == before.kf, "%s: G %u g %u past the total moved the cursor", name, G, g);
        return;
      }
      while (!(t.pk0[model_k] <= g && g < t.pk0[model_k + 1])) model_k++;
      CHECK(c[v].kw == model_k, "%s: G %u g %u wave %u: write %u, want %u", name, G, g, v, c[v].kw, model_k);
      if (c[v].kw != model_k) return;
      const ModelWrite &w = *t.w[model_k];
      uint64_t a;
      uint32_t dlen;
      w.packet(g - t.pk0[model_k], a, dlen);
      const uint32_t nfull = dlen / 512u, first = 8u * v;
      const uint32_t nfr = nfull > first ? (nfull - first < 8u ? nfull - first : 8u) : 0u;
      if (!nfr) {  // looks no slice and no fragment up; only a change of the write may have reset the hint
        CHECK(c[v].kf == (before.kw == c[v].kw ? before.kf : 0u), "%s: G %u g %u wave %u: hint %u", name, G, g, v,
              c[v].kf);
        return;
      }
      const Slice s = slice_of(t.fr0, c[v].kw);
      CHECK(s.first == t.fr0[model_k] && s.nf == w.nf(), "%s: G %u g %u: slice %u+%u", name, G, g, s.first, s.nf);
      const uint64_t ra = a + 4096u * uint64_t(v);
      const uint32_t want = w.frag(ra);
      CHECK(c[v].kf <= want, "%s: G %u g %u wave %u: hint %u past the answer %u", name, G, g, v, c[v].kf, want);
      if (c[v].kf > want) {
        c[v].kf = want;
        return;
      }
      const uint32_t got = seek_frag(SliceAt{t.at + s.first, s.nf, name}, s.nf, ra, c[v]);
      CHECK(got == want && c[v].kf == want, "%s: G %u g %u wave %u pos %llu: fragment %u, want %u", name, G, g, v,
            (unsigned long long)ra, got, want);
    };
    // wave 0's chunk shorter than 512 B of global packet g, with the cursor kept for it
    auto ragged = [&](uint32_t g, const Cursor &k) {
      uint32_t mk = 0;
      while (!(t.pk0[mk] <= g && g < t.pk0[mk + 1])) mk++;
      CHECK(k.kw == mk, "%s: G %u g %u: the ragged chunk's write %u, want %u", name, G, g, k.kw, mk);
      if (k.kw != mk) return;
      const ModelWrite &w = *t.w[mk];
      uint64_t a;
      uint32_t dlen;
      w.packet(g - t.pk0[mk], a, dlen);
      const Slice s = slice_of(t.fr0, k.kw);
      CHECK(s.first == t.fr0[mk] && s.nf == w.nf(), "%s: G %u g %u: the ragged chunk's slice", name, G, g);
      if (!(dlen % 512u) || !s.nf) return;  // ragged_gather's own condition
      const uint64_t ca = a + 512u * uint64_t(dlen / 512u);
      const uint32_t want = w.frag(ca);
      CHECK(k.kf <= want, "%s: G %u g %u: the ragged chunk's hint %u past the answer %u", name, G, g, k.kf, want);
      if (k.kf > want) return;
      const uint32_t got = frag_of(SliceAt{t.at + s.first, s.nf, name}, s.nf, ca, k.kf);
      CHECK(got == want, "%s: G %u g %u: the ragged chunk's fragment %u, want %u", name, G, g, got, want);
    };
    uint32_t g = b;
    for (uint32_t v = 0; v < 16; v++) unit(g, v), kc[v] = c[v];
    while (g < limit) {
      const uint32_t keep = model_k;
      for (uint32_t v = 0; v < 16; v++) model_k = keep, unit(g + G, v);  // the next packet's lookups first
      ragged(g, kc[0]);
      for (uint32_t v = 0; v < 16; v++) kc[v] = c[v];
      g += G;
    }
  }
}

// ---- the counters ----------------------------------------------------------------------
static void counters(const char *name, const std::vector<ModelWrite> &batch) {
  RoundCounts got, want;
  for (const ModelWrite &w : batch) {
    uint32_t hint = 0;
    for (uint64_t i = 0; i < w.npk(); i++) {
      uint64_t a;
      uint32_t dlen;
      w.packet(i, a, dlen);
      if (!dlen) continue;
      count_packet(w.at.data(), w.nf(), a, dlen, hint, got);
      const uint32_t full = dlen / 512u * 512u;
      for (uint32_t r = 0; r < full; r += 4096u) {
        const uint32_t n = w.under(a + r, a + (full - r < 4096u ? full : r + 4096u));
        want.rounds++;
        want.seamed_rounds += n > 1u;
        if (n > want.max_frags_per_round) want.max_frags_per_round = n;
      }
      if (dlen % 512u) want.seamed_ragged += w.under(a + full, a + dlen) > 1u;
    }
  }
  CHECK(got.rounds == want.rounds && got.seamed_rounds == want.seamed_rounds &&
            got.seamed_ragged == want.seamed_ragged && got.max_frags_per_round == want.max_frags_per_round,
        "counters of %s: got %llu/%llu/%llu/%u, want %llu/%llu/%llu/%u", name, (unsigned long long)got.rounds,
        (unsigned long long)got.seamed_rounds, (unsigned long long)got.seamed_ragged, got.max_frags_per_round,
        (unsigned long long)want.rounds, (unsigned long long)want.seamed_rounds,
        (unsigned long long)want.seamed_ragged, want.max_frags_per_round);
}

static void run(const char *name, const std::vector<ModelWrite> &batch) {
  Tables t;
  build(batch, t);
  for (const uint32_t G : {1u, 3u, 7u, 256u}) walk(name, t, G, t.total, 0u);
  counters(name, batch);
}

// A batch of millions of packets: every workgroup of every G walks its first
// `limit` global packets, and three workgroups of 256 walk all of it.
static void run_long(const char *name, const std::vector<ModelWrite> &batch, uint32_t limit) {
  Tables t;
  build(batch, t);
  for (const uint32_t G : {1u, 3u, 7u, 256u}) walk(name, t, G, limit, 0u);
  walk(name, t, 256u, t.total, 128u);
  counters(name, batch);
}

int main() {
  const std::vector<uint64_t> ones(1300, 1);
  const std::vector<uint64_t> many(40, 4097);  // 160 KiB: three packets, nearly every round seamed
  // a write of 1 300 one-byte fragments ahead of a write of one fragment, and the reverse
  run("ones, one", {mw(ones, 287, true), mw({70000}, 0, true)});
  run("ones, one (aligned)", {mw(ones, 0, false), mw({70000}, 287, false)});
  run("one, ones", {mw({70000}, 0, true), mw(ones, 287, true)});
  run("many, one, many", {mw(many, 287, false), mw({3}, 0, false), mw(many, 0, true)});
  {  // 300 one-packet writes of 1 to 3 fragments
    std::vector<ModelWrite> b;
    for (uint32_t k = 0; k < 300; k++) {
      std::vector<uint64_t> lens(1 + k % 3, 1 + (k * 37) % 2000);
      if (k % 5 == 0) lens.insert(lens.begin() + (k % lens.size()), 0);  // an empty fragment is no fragment
      b.push_back(mw(lens, (k % 2) ? 0u : 200u, false));
    }
    run("300 one-packet writes", b);
  }
  // writes of 0 bytes with finish between writes of many fragments (and one without: dropped)
  run("empty writes with finish", {mw(many, 287, true), mw({}, 0, true), mw({0, 0}, 0, false), mw(ones, 0, false),
                                   mw({}, 287, true), mw({}, 0, true), mw(many, 1, true)});
  // a ragged last chunk that spans two fragments, then a write whose short first packet is seamed
  run("ragged seam, short seamed head", {mw({65536 + 4096 + 100, 200}, 0, false), mw({100, 187, 5000}, 287, true)});
  run("ragged seam, short seamed head, many", {mw(many, 0, false), mw({65536 + 512 + 5, 7, 3}, 0, false),
                                               mw({1, 1, 285, 70000}, 287, true)});
  // 2^39 bytes in one fragment among tiny writes: no 32-bit position.  8.4 million packets: every workgroup walks
  // the first 70 000 (byte 2^32 of the large write is in packet 65 537), workgroups 0, 128 and 255 of 256 all of them,
  // on into the writes behind it, one of which has its second fragment past byte 2^32
  run_long("2^39 bytes among tiny ones", {mw({5}, 0, true), mw({uint64_t(1) << 39}, 287, true), mw({1, 1, 600}, 0, false),
                                     mw({(uint64_t(1) << 32) + 4097, 9000}, 0, false), mw({3}, 0, true)}, 70000u);
  std::printf("%llu checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
