// Stand-alone check of the MD5CRC streams library's cursor on the CPU: the
// functions of md5crc_streams_lookup.h that digest_streams_kernel runs with one
// lane per entry, fed with probe_entry's descriptor (read_batch_layout.h,
// md5crc_streams_internal.h: regions_of), against a brute-force
// frame::frame_step walk of the same stream.  The cursor must yield exactly the
// concatenated CRC regions: every address inside a region, every region byte
// once.  Then the whole digest as the kernel forms it, compiled for the host
// (the cursor plus md5_core.h), against a plain byte-wise MD5 of that
// concatenation.  Built with -fsanitize=address,undefined by
// tests/test_md5crc_streams_cpu.py and run as a child process; nothing of it is
// loaded into Python.  A stream ends exactly where its allocation does, at
// every residue mod 4 of its first byte, and the loads are the kernel's three
// kinds (an aligned word, two aligned words joined, bytes), so a read outside
// [stream, stream + consumed) is the sanitizer's or the test's own to report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "md5_core.h"
#include "md5crc_streams_internal.h"
#include "md5crc_streams_lookup.h"
#include "read_batch_layout.h"

using namespace hdfs_md5crc_streams;
namespace rb = hdfs_read_batch;
namespace frame = hdfs_crc32c::frame;

static int failures = 0;
static unsigned long long checks = 0;
#define CHECK(c, ...)                                 \
  do {                                                \
    checks++;                                         \
    if (!(c)) {                                       \
      if (++failures < 30) {                          \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

struct Spec {
  uint32_t dlen;
  int64_t off, seq;
  bool last;
  int sync;  // -1: the header has no syncBlock
};

static void be(uint8_t *p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = uint8_t(v >> (8 * (n - 1 - i)));
}
static void le(uint8_t *p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = uint8_t(v >> (8 * i));
}

// The header bytes of a packet, written out by hand.  -> their count.
static uint32_t put_header(uint8_t *p, int proto, const Spec &s) {
  const uint32_t ncrc = (s.dlen + 511u) / 512u;
  be(p, s.dlen + 4u * ncrc + 4u, 4);
  if (proto == HDFS_CRC32C_PROTO_V1) {
    be(p + 4, uint64_t(s.off), 8);
    be(p + 12, uint64_t(s.seq), 8);
    p[20] = s.last ? 1 : 0;
    be(p + 21, s.dlen, 4);
    return 25;
  }
  const uint32_t hlen = s.sync < 0 ? 25u : 27u;
  be(p + 4, hlen, 2);
  uint8_t *q = p + 6;
  q[0] = 0x09;
  le(q + 1, uint64_t(s.off), 8);
  q[9] = 0x11;
  le(q + 10, uint64_t(s.seq), 8);
  q[18] = 0x18;
  q[19] = s.last ? 1 : 0;
  q[20] = 0x25;
  le(q + 21, s.dlen, 4);
  if (s.sync >= 0) {
    q[25] = 0x28;
    q[26] = uint8_t(s.sync);
  }
  return 6 + hlen;
}

static uint64_t wire_bytes(int proto, const Spec &s) {
  uint8_t h[40];
  return put_header(h, proto, s) + 4ull * ((s.dlen + 511u) / 512u) + s.dlen;
}

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint8_t next_byte() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return uint8_t(g_seed >> 56);
}

// K packets of `body` bytes from block offset 0, then a packet of `ragged`
// bytes (0: none), then the empty last packet (or the last flag on the final
// data packet).  The CRC regions hold pseudo-random bytes, the data is 0x5A.
static std::vector<uint8_t> build(int proto, uint32_t body, uint32_t K, uint32_t ragged, bool empty_last, int sync) {
  std::vector<Spec> v;
  int64_t off = 0;
  for (uint32_t k = 0; k < K; k++, off += body) v.push_back(Spec{body, off, int64_t(k), false, sync});
  if (ragged) {
    v.push_back(Spec{ragged, off, int64_t(K), false, sync});
    off += ragged;
  }
  if (empty_last)
    v.push_back(Spec{0, off, int64_t(v.size()), true, -1});
  else if (!v.empty())
    v.back().last = true;
  std::vector<uint8_t> out;
  for (const Spec &s : v) {
    uint8_t h[40];
    const uint32_t hb = put_header(h, proto, s);
    out.insert(out.end(), h, h + hb);
    for (uint32_t i = 0; i < 4u * ((s.dlen + 511u) / 512u); i++) out.push_back(next_byte());
    out.insert(out.end(), s.dlen, uint8_t(0x5A));
  }
  return out;
}

struct Bytes {
  const uint8_t *s;
  const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

// ---- a plain MD5, byte-wise padding ---------------------------------------------------
static void md5_plain(const uint8_t *p, uint64_t len, uint8_t out[16]) {
  using namespace hdfs_md5crc;
  uint32_t st[4], m[16];
  md5_init(st);
  std::vector<uint8_t> msg(p, p + len);
  msg.push_back(0x80);
  while (msg.size() % 64 != 56) msg.push_back(0);
  for (int k = 0; k < 8; k++) msg.push_back(uint8_t((len << 3) >> (8 * k)));
  for (size_t o = 0; o < msg.size(); o += 64) {
    for (int j = 0; j < 16; j++)
      m[j] = uint32_t(msg[o + 4 * j]) | uint32_t(msg[o + 4 * j + 1]) << 8 | uint32_t(msg[o + 4 * j + 2]) << 16 |
             uint32_t(msg[o + 4 * j + 3]) << 24;
    md5_block(st, m);
  }
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 4; k++) out[4 * j + k] = uint8_t(st[j] >> (8 * k));
}

// ---- the kernel's loads, on host memory --------------------------------------------------
// seen[i]: how often byte i of the stream was handed out as a CRC byte; in[i]:
// whether it lies in a region (the walk's records say so).
struct Host {
  const Regions &r;
  std::vector<uint8_t> &seen;
  const std::vector<uint8_t> &in;
  const char *name;

  const uint8_t *at(uint64_t off) const { return reinterpret_cast<const uint8_t *>(uintptr_t(r.base)) + off; }
  uint32_t aligned_word(const uint8_t *p) const {
    CHECK((reinterpret_cast<uintptr_t>(p) & 3u) == 0u, "%s: an unaligned word load", name);
    uint32_t x;
    std::memcpy(&x, p, 4);
    return x;
  }
  void mark(uint64_t off) const {
    for (uint64_t i = off; i < off + 4; i++) {
      CHECK(i < in.size() && in[i], "%s: byte %llu is outside every region", name, (unsigned long long)i);
      if (i < seen.size()) seen[i]++;
    }
  }
  void word(uint64_t off, uint32_t &lo, uint32_t &hi, uint32_t &a) const {
    mark(off);
    const uint8_t *A = at(off);
    const uint64_t addr = reinterpret_cast<uintptr_t>(A);
    a = uint32_t(addr) & 3u;
    if (a != 0u && !aligned_cover_ok(r, off, a, 1u)) {
      lo = by_bytes(A[0], A[1], A[2], A[3]);
      hi = a = 0u;
      return;
    }
    lo = aligned_word(reinterpret_cast<const uint8_t *>(uintptr_t(lo_address(addr))));
    hi = aligned_word(reinterpret_cast<const uint8_t *>(uintptr_t(hi_address(addr))));
  }
  void span(uint64_t off, Loaded &x) const {
    const uint8_t *A = at(off);
    const uint32_t a = uint32_t(reinterpret_cast<uintptr_t>(A)) & 3u;
    if (a != 0u && !aligned_cover_ok(r, off, a, kBlockWords)) {
      x.sh = 0u;
      for (uint32_t j = 0; j < kBlockWords; j++) {
        uint32_t aj;
        word(off + 4u * j, x.lo[j], x.hi[j], aj);
        x.sh |= aj << (2u * j);
      }
      return;
    }
    for (uint32_t j = 0; j < kBlockWords; j++) {
      mark(off + 4u * j);
      x.lo[j] = aligned_word(A - a + 4u * j);
    }
    x.hi[kBlockWords - 1] = aligned_word(A - a + 4u * (a ? kBlockWords : kBlockWords - 1u));
    for (uint32_t j = 0; j + 1u < kBlockWords; j++) x.hi[j] = x.lo[j + 1];
    x.sh = a * 0x55555555u;
  }
};
struct SpanOf {
  const Host &h;
  void operator()(uint64_t off, Loaded &x) const { h.span(off, x); }
};
struct WordOf {
  const Host &h;
  void operator()(uint64_t off, uint32_t &lo, uint32_t &hi, uint32_t &a) const { h.word(off, lo, hi, a); }
};

// The digest as the kernel forms it; words: the message words the cursor gave.
static void digest_like_the_kernel(const Regions &r, const Host &h, std::vector<uint32_t> &words, uint8_t out[16]) {
  using namespace hdfs_md5crc;
  Cursor c = start(r);
  uint32_t st[4];
  md5_init(st);
  CHECK(r.nblk == md5_words_blocks(r.nwords), "%s: %u blocks for %llu words", h.name, r.nblk,
        (unsigned long long)r.nwords);
  for (uint32_t b = 0; b < r.nblk; b++) {
    uint32_t m[16];
    Loaded x;
    block_words(r, c, b, SpanOf{h}, WordOf{h}, x);
    message_words(x, m);
    for (uint32_t j = 0; j < 16; j++)
      if (16ull * b + j < r.nwords) words.push_back(m[j]);
    if (b + 1 == r.nblk) {
      m[14] = uint32_t(r.nwords << 5);
      m[15] = uint32_t(r.nwords >> 27);
    }
    md5_block(st, m);
  }
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 4; k++) out[4 * j + k] = uint8_t(st[j] >> (8 * k));
}

static unsigned long long regular_cases = 0;

// One stream at residue `res`, `cut` bytes short of its end.
static void one(const char *name, int proto, const std::vector<uint8_t> &all, uint64_t cut, uint32_t res,
                bool want_regular = true) {
  const uint64_t len = all.size() - cut;
  // operator new gives 16-byte alignment: the stream starts res bytes in and ends where the allocation does
  uint8_t *tight = new uint8_t[res + len ? res + len : 1];
  uint8_t *s = tight + res;
  if ((reinterpret_cast<uintptr_t>(tight) & 3u) != 0u) {
    CHECK(false, "%s: the allocator's alignment", name);
    delete[] tight;
    return;
  }
  if (len) std::memcpy(s, all.data(), len);
  // the walk: records, the concatenated CRC regions, the region map
  std::vector<uint8_t> want, in(len, 0), seen(len, 0);
  uint64_t pos = 0, npk = 0, payload = 0;
  int error = 0;
  while (pos < len) {
    hdfs_crc32c_packet k;
    uint64_t total = 0;
    const int r = frame::frame_step(s + pos, len - pos, pos, proto, 512, HDFS_CRC32C_CSUM_CRC32C, k, total);
    if (r == frame::kStepMore) break;
    npk++;
    if (k.error) {
      error = k.error;
      break;
    }
    for (uint64_t i = 0; i < uint64_t(k.crc_len); i++) {
      want.push_back(s[pos + k.header_len + i]);
      in[pos + k.header_len + i] = 1;
    }
    payload += uint64_t(k.data_len);
    pos += total;
    if (r == frame::kStepStop) break;
  }
  rb::Desc d;
  std::memset(&d, 0xEE, sizeof(d));
  const bool regular = rb::probe_entry(Bytes{s}, len, ~0ull, proto, 512, HDFS_CRC32C_CSUM_CRC32C, false, 0, d);
  CHECK(regular == want_regular, "%s (proto %d, residue %u): regular %d", name, proto, res, int(regular));
  if (regular) {
    regular_cases++;
    const Regions r = regions_of(d, s, 7u);
    CHECK(!error && d.consumed == pos && d.npk == npk && d.delivered == payload, "%s: the probe and the walk", name);
    CHECK(r.nwords * 4u == want.size() && r.limit == pos && r.entry == 7u, "%s: %llu words, the walk has %zu bytes",
          name, (unsigned long long)r.nwords, want.size());
    const Host h{r, seen, in, name};
    std::vector<uint32_t> words;
    uint8_t got[16], plain[16];
    digest_like_the_kernel(r, h, words, got);
    CHECK(words.size() * 4u == want.size() && (want.empty() || !std::memcmp(words.data(), want.data(), want.size())),
          "%s (proto %d, residue %u): the cursor's words are not the regions' bytes", name, proto, res);
    bool once = true;
    for (uint64_t i = 0; i < len; i++) once = once && seen[i] == in[i];
    CHECK(once, "%s (proto %d, residue %u): a region byte not produced exactly once", name, proto, res);
    md5_plain(want.data(), want.size(), plain);
    CHECK(!std::memcmp(got, plain, 16), "%s (proto %d, residue %u): the digest", name, proto, res);
  }
  delete[] tight;
}

// The fallback's descriptor: one region of n words in scratch.
static void one_region(uint32_t n) {
  std::vector<uint8_t> crcs(n ? 4u * n : 1u);
  for (uint32_t i = 0; i < 4u * n; i++) crcs[i] = next_byte();
  uint8_t *s = new uint8_t[n ? 4u * n : 1u];
  std::memcpy(s, crcs.data(), 4u * n);
  Regions r = Regions{};
  r.base = reinterpret_cast<uintptr_t>(s);
  r.limit = 4ull * n;
  r.nwords = n;
  r.ntail = 1;
  r.tail_words0 = n;
  r.nblk = uint32_t(hdfs_md5crc::md5_words_blocks(n));
  std::vector<uint8_t> in(4u * n, 1), seen(4u * n, 0);
  const Host h{r, seen, in, "one region"};
  std::vector<uint32_t> words;
  uint8_t got[16], plain[16];
  digest_like_the_kernel(r, h, words, got);
  md5_plain(crcs.data(), 4ull * n, plain);
  CHECK(words.size() == n && !std::memcmp(got, plain, 16), "one region of %u words", n);
  bool once = true;
  for (uint32_t i = 0; i < 4u * n; i++) once = once && seen[i] == 1;
  CHECK(once, "one region of %u words: a byte not produced exactly once", n);
  delete[] s;
}

// A stream of 2^39 bytes that exists only as arithmetic: K full packets, a
// shorter one, the empty last one; at(pos) composes the header that starts
// there.
struct Sparse {
  int proto;
  uint64_t stride, K;
  uint32_t dlen, tail_dlen;
  mutable uint8_t buf[64];
  const uint8_t *operator()(uint64_t pos) const {
    std::memset(buf, 0, sizeof(buf));
    const uint64_t k = pos / stride;
    Spec s{dlen, int64_t(k * dlen), int64_t(k), false, -1};
    if (k < K && pos % stride == 0) {
      put_header(buf, proto, s);
    } else if (pos == K * stride) {
      s.dlen = tail_dlen;
      put_header(buf, proto, s);
    } else if (pos == K * stride + wire_bytes(proto, Spec{tail_dlen, 0, 0, false, -1})) {
      s = Spec{0, int64_t(K * dlen + tail_dlen), int64_t(K + 1), true, -1};
      put_header(buf, proto, s);
    }
    return buf;
  }
};

int main() {
  {  // the plain MD5 this file compares with, against RFC 1321's test suite
    uint8_t d[16];
    const uint8_t empty[16] = {0xd4, 0x1d, 0x8c, 0xd9, 0x8f, 0x00, 0xb2, 0x04, 0xe9, 0x80, 0x09, 0x98, 0xec, 0xf8, 0x42, 0x7e};
    const uint8_t abc[16] = {0x90, 0x01, 0x50, 0x98, 0x3c, 0xd2, 0x4f, 0xb0, 0xd6, 0x96, 0x3f, 0x7d, 0x28, 0xe1, 0x7f, 0x72};
    md5_plain(nullptr, 0, d);
    CHECK(!std::memcmp(d, empty, 16), "MD5 of the empty message");
    md5_plain(reinterpret_cast<const uint8_t *>("abc"), 3, d);
    CHECK(!std::memcmp(d, abc, 16), "MD5 of abc");
  }
  const uint32_t raggeds[] = {0, 1, 511, 513, 1300};
  struct Body {
    uint32_t dlen;
    std::vector<uint32_t> counts;
  };
  // 512-byte packets: a word each, so every total of 1, 13 .. 17 and 16 k + {0, 13, 14, 15} with the tails'
  // 0 .. 3 words; 5 120-byte packets: ten words, a block begins in one packet and ends in another every trip;
  // 64 KiB packets: 128 words, never
  const Body bodies[] = {{512, {1, 2, 13, 14, 15, 16, 17, 29, 30, 31, 32, 33, 48}},
                         {5120, {1, 2, 3, 8, 16}},
                         {65536, {1, 2, 3}}};
  uint32_t res = 0;
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2})
    for (const int sync : {-1, 1}) {
      if (sync >= 0 && proto == HDFS_CRC32C_PROTO_V1) continue;
      for (const Body &b : bodies)
        for (const uint32_t K : b.counts)
          for (const uint32_t ragged : raggeds)
            for (const bool empty_last : {true, false}) {
              const std::vector<uint8_t> all = build(proto, b.dlen, K, ragged, empty_last, sync);
              char name[96];
              std::snprintf(name, sizeof(name), "[%u]*%u + [%u]%s%s", b.dlen, K, ragged, empty_last ? " + empty" : "",
                            sync >= 0 ? ", syncBlock" : "");
              // every residue for the small streams, one in turn for the large ones
              for (uint32_t r4 = 0; r4 < 4; r4++) {
                if (all.size() > 100000 && r4 != res % 4) continue;
                // the probe's rule: a packet behind the run is shorter than the run's (the others are the
                // main library's to frame, and the library's fallback)
                const bool shape = ragged < b.dlen;
                one(name, proto, all, 0, r4, shape);
                // a cut packet at the end: the walk ends ahead of it (the empty one, else the shorter one,
                // else the run's last), and a complete packet must be left
                one(name, proto, all, 7, r4, empty_last ? shape : ragged ? true : K > 1);
              }
              res++;
            }
    }
  CHECK(regular_cases > 2000, "only %llu regular cases", regular_cases);
  // what the probe leaves to the main library stays irregular here too
  one("[40000]*5", 2, build(2, 40000, 5, 0, true, -1), 0, 1, false);
  one("only the empty last packet", 2, build(2, 512, 0, 0, true, -1), 0, 3, false);
  // the fallback's descriptor
  for (const uint32_t n : {0u, 1u, 13u, 14u, 15u, 16u, 17u, 29u, 30u, 31u, 32u, 45u, 46u, 47u, 48u, 1000u}) one_region(n);
  // 2^39 bytes: the counts
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2}) {
    Sparse sp;
    sp.proto = proto;
    sp.dlen = 65536;
    sp.tail_dlen = 1000;
    sp.stride = wire_bytes(proto, Spec{65536, 0, 0, false, -1});
    const uint64_t len = 1ull << 39;
    const uint64_t tail = wire_bytes(proto, Spec{1000, 0, 0, false, -1}) + wire_bytes(proto, Spec{0, 0, 0, true, -1});
    sp.K = (len - tail) / sp.stride;
    rb::Desc d;
    const bool regular = rb::probe_entry(sp, len, ~0ull, proto, 512, HDFS_CRC32C_CSUM_CRC32C, false, 0, d);
    CHECK(regular, "2^39 bytes: regular");
    const Regions r = regions_of(d, nullptr, 0u);
    CHECK(r.nwords == sp.K * 128u + 2u && r.nwords > (1ull << 29) && r.limit == sp.K * sp.stride + tail,
          "2^39 bytes: %llu words", (unsigned long long)r.nwords);
    CHECK(r.nblk == (r.nwords + 18u) / 16u && r.nbody == sp.K - 1u && r.wpp == 128u && r.ntail == 3u &&
              r.tail_words0 == 128u && r.tail_words1 == 2u && r.tail_words2 == 0u,
          "2^39 bytes: the descriptor");
    CHECK(r.tail_off0 == (sp.K - 1u) * sp.stride + r.hb0 && r.tail_off0 > (1ull << 38), "2^39 bytes: the tail");
    // the first packets' offsets, by the cursor and by multiplication
    Cursor c = start(r);
    bool ok = true;
    for (uint64_t i = 0; i < 5000; i++) {
      settle(r, c);
      ok = ok && span_ahead(c) && take_span(c) == (i / 8u) * sp.stride + r.hb0 + 64u * (i % 8u);
    }
    CHECK(ok, "2^39 bytes: the cursor's first spans");
  }
  std::printf("%llu checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
