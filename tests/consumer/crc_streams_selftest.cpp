// Stand-alone check of the CRC streams library's arithmetic on the CPU: the
// functions of crc_streams_lookup.h that fold_packets_kernel and
// reduce_entries_kernel run, lane by lane as the kernels run them, fed with
// probe_entry's descriptor (read_batch_layout.h, crc_streams_internal.h:
// shape_of) and, for every stream, with the packets a brute-force
// frame::frame_step walk finds (the described-packet path), against a
// byte-wise CRC of the payload for both polynomials.  The streams carry their
// chunks' own CRCs.  Also: the multiply against Gf2::apply, x^(8n) up to 2^62
// against zeros_op, the file combine against the CRC of the concatenation, and
// a stream of 2^39 bytes that exists only as arithmetic.  Built with
// -fsanitize=address,undefined by tests/test_crc_streams_cpu.py and run as a
// child process; nothing of it is loaded into Python.  Every CRC region is read
// through `Region`, which refuses an index outside the region.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crc32c_tables.h"
#include "crc_streams_internal.h"
#include "crc_streams_lookup.h"
#include "read_batch_layout.h"

using namespace hdfs_crc_streams;
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

// ---- a byte-wise CRC ----------------------------------------------------------------------
// Four bytes a step where there are four (crc32c_tables.h's slicing tables, which
// main() checks against the check values of both polynomials and against the
// one-byte loop).
struct ByteCrc {
  uint32_t poly, t[4][256];
  explicit ByteCrc(uint32_t p) : poly(p) { hdfs_crc32c::make_slicing4(t, p); }
  uint32_t operator()(const uint8_t *p, size_t n, uint32_t crc = 0) const {
    crc = ~crc;
    size_t i = 0;
    for (; i + 4 <= n; i += 4) {
      uint32_t w;
      std::memcpy(&w, p + i, 4);
      crc ^= w;
      crc = t[3][crc & 0xFF] ^ t[2][(crc >> 8) & 0xFF] ^ t[1][(crc >> 16) & 0xFF] ^ t[0][crc >> 24];
    }
    for (; i < n; i++) crc = t[0][(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return ~crc;
  }
  uint32_t bitwise(const uint8_t *p, size_t n) const {
    uint32_t crc = ~0u;
    for (size_t i = 0; i < n; i++) {
      crc ^= p[i];
      for (int b = 0; b < 8; b++) crc = (crc >> 1) ^ (poly & (0u - (crc & 1u)));
    }
    return ~crc;
  }
};

// ---- streams ----------------------------------------------------------------------------
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

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint8_t next_byte() {
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return uint8_t(g_seed >> 56);
}

static void fill(std::vector<uint8_t> &v) {
  size_t i = 0;
  for (; i + 8 <= v.size(); i += 8) {
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    const uint64_t x = g_seed ^ (g_seed >> 29);
    std::memcpy(&v[i], &x, 8);
  }
  for (; i < v.size(); i++) v[i] = next_byte();
}

// K packets of `body` bytes from block offset 0, then a packet of `ragged`
// bytes (0: none), then the empty last packet (or the last flag on the final
// data packet) or, with `cut`, the header and 7 more bytes of one more packet.
// The data is pseudo-random, the CRC regions hold its chunks' CRCs; `payload` gets
// the data of the complete packets.
static std::vector<uint8_t> build(const ByteCrc &crc, int proto, uint32_t body, uint32_t K, uint32_t ragged,
                                  bool empty_last, int sync, bool cut, std::vector<uint8_t> &payload) {
  std::vector<Spec> v;
  int64_t off = 0;
  for (uint32_t k = 0; k < K; k++, off += body) v.push_back(Spec{body, off, int64_t(k), false, sync});
  if (ragged) {
    v.push_back(Spec{ragged, off, int64_t(K), false, sync});
    off += ragged;
  }
  if (empty_last && !cut)
    v.push_back(Spec{0, off, int64_t(v.size()), true, -1});
  else if (!v.empty() && !cut)
    v.back().last = true;
  if (cut) v.push_back(Spec{body, off, int64_t(v.size()), false, sync});
  std::vector<uint8_t> out;
  payload.clear();
  for (size_t i = 0; i < v.size(); i++) {
    const Spec &s = v[i];
    uint8_t h[40];
    const uint32_t hb = put_header(h, proto, s);
    out.insert(out.end(), h, h + hb);
    if (cut && i + 1 == v.size()) {  // the stream ends 7 bytes into this packet's CRCs and data
      for (int j = 0; j < 7; j++) out.push_back(next_byte());
      break;
    }
    std::vector<uint8_t> data(s.dlen);
    fill(data);
    for (uint32_t c = 0; c * 512u < s.dlen; c++) {
      uint8_t w[4];
      be(w, crc(data.data() + 512u * c, s.dlen - 512u * c < 512u ? s.dlen - 512u * c : 512u), 4);
      out.insert(out.end(), w, w + 4);
    }
    out.insert(out.end(), data.begin(), data.end());
    payload.insert(payload.end(), data.begin(), data.end());
  }
  return out;
}

struct Bytes {
  const uint8_t *s;
  const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

// A packet's CRC region in host memory: word i as the kernel's buffer load
// gives it, zero outside (and counted as a failure: the kernel's lanes ask only
// for kNoChunk outside, which never gets here).
struct Region {
  const uint8_t *p;
  uint32_t ncrc;
  std::vector<uint8_t> *seen;
  uint32_t word(uint32_t i) const {
    CHECK(i < ncrc, "word %u of a region of %u", i, ncrc);
    if (i >= ncrc) return 0u;
    if (seen) (*seen)[i]++;
    uint32_t w;
    std::memcpy(&w, p + 4u * size_t(i), 4);
    return w;
  }
};

// fold_packets_kernel's fold of one packet, lane by lane.
static uint32_t fold_packet(const Region &rg, uint32_t dlen, const uint32_t *mult, const char *name) {
  const uint32_t poly = mult[kMultPoly], mstep = mult[kMultStep];
  const Chunks ch = chunks_of(rg.ncrc, dlen, mult[kMultChunk]);
  std::vector<uint8_t> seen(rg.ncrc, 0);
  Region r = rg;
  r.seen = &seen;
  uint32_t front = 0;
  for (uint32_t lane = 0; lane < kLanes; lane++) {
    uint32_t a = 0;
    for (uint32_t s = 0; s < ch.steps; s++) {
      const uint32_t i = chunk_at(ch, s, lane);
      CHECK(i == kNoChunk || i < ch.front, "%s: lane %u step %u takes chunk %u of %u", name, lane, s, i, ch.front);
      a = fold_step(a, i != kNoChunk ? r.word(i) : 0u, s, mstep, poly);
    }
    front ^= mulmod(a, mult[kMultLane + lane], poly);
  }
  for (uint32_t i = 0; i < ch.front; i++) CHECK(seen[i] == 1, "%s: chunk %u taken %u times", name, i, seen[i]);
  const uint32_t last = rg.ncrc ? r.word(rg.ncrc - 1u) : 0u;
  return packet_crc(ch, front, last, xpow8(mult + kMultPow2, ch.last_len, poly), poly);
}

// reduce_entries_kernel's reduce of one entry, lane by lane.  sh: the regular
// entry's shape, or NULL: the described path with recs.
static uint32_t reduce_entry(const Shape *sh, const std::vector<PktRec> &recs, const std::vector<uint32_t> &cp,
                             uint32_t npk, const uint32_t *mult, const char *name) {
  const uint32_t poly = mult[kMultPoly];
  const uint32_t *pow2 = mult + kMultPow2;
  Shape z = Shape{};
  if (sh) z = *sh;
  const uint32_t x0 = xpow8(pow2, z.dlen0, poly), xt0 = xpow8(pow2, z.tail0, poly), xt1 = xpow8(pow2, z.tail1, poly),
                 xt2 = xpow8(pow2, z.tail2, poly);
  uint32_t out = 0, next = 0;
  for (uint32_t lane = 0; lane < kLanes; lane++) {
    const uint32_t first = run_first(npk, lane), end = first + run_count(npk, lane);
    CHECK(first == next && end <= npk, "%s: lane %u runs [%u, %u) behind %u of %u", name, lane, first, end, next, npk);
    next = end;
    uint32_t acc = 0;
    for (uint32_t i = first; i < end; i++) {
      uint32_t m;
      if (!sh) {
        m = xpow8(pow2, recs[i].dlen, poly);
      } else {
        const uint32_t t = i - z.nbody;
        m = i < z.nbody ? x0 : t == 0u ? xt0 : t == 1u ? xt1 : xt2;
      }
      acc = mulmod(acc, m, poly) ^ cp[i];
    }
    uint64_t behind = 0;
    if (end > first) behind = !sh ? recs[end - 1u].after : bytes_before(z, npk) - bytes_before(z, end);
    out ^= advance(pow2, acc, behind, poly);
  }
  CHECK(next == npk, "%s: the runs end at %u of %u", name, next, npk);
  return out;
}

static void one_stream(const ByteCrc &crc, int ctype, int proto, uint32_t body, uint32_t K, uint32_t ragged,
                       bool empty_last, int sync, bool cut, const uint32_t *mult) {
  char name[160];
  std::snprintf(name, sizeof(name), "poly %08x v%d body %u x %u ragged %u empty %d sync %d cut %d", crc.poly, proto,
                body, K, ragged, int(empty_last), sync, int(cut));
  std::vector<uint8_t> payload;
  const std::vector<uint8_t> built = build(crc, proto, body, K, ragged, empty_last, sync, cut, payload);
  // the stream ends where its allocation does
  std::vector<uint8_t> s(built);
  const uint32_t want = crc(payload.data(), payload.size());

  // the described path: a brute-force walk's packets
  std::vector<PktRec> recs;
  uint64_t pos = 0;
  while (pos < s.size()) {
    hdfs_crc32c_packet k;
    uint64_t total = 0;
    const int r = frame::frame_step(s.data() + pos, s.size() - pos, pos, proto, 512, ctype, k, total);
    if (r == frame::kStepMore) break;
    CHECK(!k.error, "%s: packet error %d at %llu", name, k.error, (unsigned long long)pos);
    if (k.error) return;
    if (k.crc_len > 0)
      recs.push_back(PktRec{uintptr_t(s.data() + pos + k.header_len), 0u, uint32_t(k.crc_len) / 4u,
                            uint32_t(k.data_len)});
    pos += total;
    if (r == frame::kStepStop) break;
  }
  uint64_t after = 0;
  for (size_t i = recs.size(); i-- > 0;) {
    recs[i].after = after;
    after += recs[i].dlen;
  }
  CHECK(after == payload.size(), "%s: the walk's payload %llu, built %zu", name, (unsigned long long)after,
        payload.size());
  std::vector<uint32_t> cp(recs.size());
  size_t at = 0;
  for (size_t i = 0; i < recs.size(); i++) {
    cp[i] = fold_packet(Region{reinterpret_cast<const uint8_t *>(uintptr_t(recs[i].addr)), recs[i].ncrc, nullptr},
                        recs[i].dlen, mult, name);
    const uint32_t pc = crc(payload.data() + at, recs[i].dlen);
    CHECK(cp[i] == pc, "%s: packet %zu folds to %08x, its bytes' CRC is %08x", name, i, cp[i], pc);
    at += recs[i].dlen;
  }
  const uint32_t got_d = recs.empty() ? 0u : reduce_entry(nullptr, recs, cp, uint32_t(recs.size()), mult, name);
  CHECK(got_d == want, "%s: described path %08x, byte-wise %08x", name, got_d, want);

  // the kernel path: the probe's descriptor
  rb::Desc d;
  const bool regular = rb::probe_entry(Bytes{s.data()}, s.size(), ~uint64_t(0), proto, 512, ctype, false, 0, d);
  const bool expect_regular = K >= 1 && (!ragged || ragged < body);
  CHECK(regular == expect_regular, "%s: regular %d, expected %d", name, int(regular), int(expect_regular));
  if (!regular) return;
  const Shape sh = shape_of(d);
  CHECK(d.delivered == payload.size() && bytes_before(sh, d.npk) == d.delivered, "%s: delivered %llu of %zu", name,
        (unsigned long long)d.delivered, payload.size());
  std::vector<uint32_t> ck(d.npk);
  for (uint32_t i = 0; i < d.npk; i++) {
    const rb::PacketAt p = rb::packet_of(d, i);
    CHECK(p.stream_off + p.hb + 4ull * rb::crc_count(p.dlen) <= d.consumed, "%s: packet %u's region leaves the stream",
          name, i);
    ck[i] = fold_packet(Region{s.data() + p.stream_off + p.hb, rb::crc_count(p.dlen), nullptr}, p.dlen, mult, name);
  }
  const uint32_t got_k = reduce_entry(&sh, recs, ck, d.npk, mult, name);
  CHECK(got_k == want, "%s: kernel path %08x, byte-wise %08x", name, got_k, want);
}

static void streams(int ctype, uint32_t poly) {
  const ByteCrc crc(poly);
  uint32_t mult[kMultWords];
  make_multipliers(mult, poly, 512);
  const uint32_t bodies[] = {512, 5120, 65536}, tails[] = {0, 1, 511, 513, 1300}, counts[] = {1, 2, 63, 64, 65, 129};
  const int protos[][2] = {{HDFS_CRC32C_PROTO_V1, -1}, {HDFS_CRC32C_PROTO_V2, -1}, {HDFS_CRC32C_PROTO_V2, 1}};
  unsigned n = 0;
  for (const auto &pr : protos)
    for (uint32_t body : bodies)
      for (uint32_t tail : tails)
        for (uint32_t K : counts)
          for (int empty_last = 0; empty_last < 2; empty_last++, n++)
            one_stream(crc, ctype, pr[0], body, K, tail, empty_last != 0, pr[1], n % 5u == 2u, mult);
  // no complete packet, and only the empty last one
  one_stream(crc, ctype, HDFS_CRC32C_PROTO_V2, 512, 0, 0, false, -1, true, mult);
  one_stream(crc, ctype, HDFS_CRC32C_PROTO_V2, 512, 0, 0, true, -1, false, mult);
}

// ---- the arithmetic alone ---------------------------------------------------------------
static void arithmetic(uint32_t poly) {
  using hdfs_crc32c::Gf2;
  using hdfs_crc32c::zeros_op;
  uint32_t mult[kMultWords];
  make_multipliers(mult, poly, 512);
  const uint32_t *pow2 = mult + kMultPow2;
  // the multiply against the operator: v * x^(8n) == Z_n(v)
  for (uint64_t n : {0ull, 1ull, 3ull, 4ull, 511ull, 512ull, 513ull, 65536ull, 0xFFFFFFFFull, 1ull << 32, 1ull << 40}) {
    const Gf2 z = zeros_op(n, poly);
    const uint32_t x = z.apply(kOne);
    CHECK(xpow8(pow2, n, poly) == x, "x^(8 * %llu)", (unsigned long long)n);
    for (int k = 0; k < 64; k++) {
      const uint32_t v = uint32_t(next_byte()) << 24 | uint32_t(next_byte()) << 16 | uint32_t(next_byte()) << 8 |
                         next_byte();
      CHECK(mulmod(v, x, poly) == z.apply(v) && mulmod(x, v, poly) == z.apply(v), "%08x * x^(8 * %llu)", v,
            (unsigned long long)n);
      CHECK(advance(pow2, v, n, poly) == z.apply(v), "advance %08x by %llu", v, (unsigned long long)n);
    }
  }
  CHECK(mulmod(kOne, 0x12345678u, poly) == 0x12345678u && mulmod(0u, 0xFFFFFFFFu, poly) == 0u, "1 and 0");
  // x^(8n) for n up to 2^62
  for (int b = 0; b <= 62; b++)
    for (uint64_t n : {1ull << b, (1ull << b) - 1u, (1ull << b) | 0x5A5A5A5A5ull >> (b & 31)}) {
      n &= 0x7FFFFFFFFFFFFFFFull;
      CHECK(xpow8(pow2, n, poly) == zeros_op(n, poly).apply(kOne), "x^(8 * %llu)", (unsigned long long)n);
    }
  // the lane and step multipliers
  for (uint32_t l = 0; l < kLanes; l++)
    CHECK(mult[kMultLane + l] == zeros_op(512ull * (63u - l), poly).apply(kOne), "lane multiplier %u", l);
  CHECK(mult[kMultStep] == zeros_op(512ull * 64u, poly).apply(kOne), "step multiplier");
  CHECK(from_wire(0x44332211u) == 0x11223344u, "from_wire");
  // the file combine: acc = Z_len(acc) ^ crc over pieces of unequal length
  const ByteCrc crc(poly);
  std::vector<uint8_t> all;
  uint32_t acc = 0;
  for (size_t len : {size_t(1), size_t(0), size_t(513), size_t(70000), size_t(3), size_t(65536)}) {
    std::vector<uint8_t> piece(len);
    for (uint8_t &b : piece) b = next_byte();
    acc = zeros_op(len, poly).apply(acc) ^ crc(piece.data(), len);
    all.insert(all.end(), piece.begin(), piece.end());
    CHECK(acc == crc(all.data(), all.size()), "combine after %zu bytes", all.size());
  }
  // a stream of 2^39 bytes that exists only as arithmetic: 2^23 packets of 64 KiB whose CRCs are all `c`,
  // reduced as the kernel does, against the closed form c * (x^(8 d N) - 1) / (x^(8 d) - 1) summed by doubling
  const uint32_t c = 0xDEADBEEFu, npk = 1u << 23, dlen = 65536;
  Shape sh = Shape{};
  sh.nbody = npk - 1u;
  sh.ntail = 1;
  sh.dlen0 = sh.tail0 = dlen;
  CHECK(bytes_before(sh, npk) == 1ull << 39, "2^39 bytes");
  const uint32_t x0 = xpow8(pow2, dlen, poly);
  uint32_t out = 0;
  // one lane's Horner sum over q equal packets is the same for every lane: S_q = sum_{j<q} c x0^j
  const uint32_t q = npk / kLanes;
  uint32_t sq = 0;
  for (uint32_t j = 0; j < q; j++) sq = mulmod(sq, x0, poly) ^ c;
  for (uint32_t lane = 0; lane < kLanes; lane++) {
    CHECK(run_count(npk, lane) == q && run_first(npk, lane) == lane * q, "lane %u's run", lane);
    const uint64_t behind = bytes_before(sh, npk) - bytes_before(sh, run_first(npk, lane) + q);
    CHECK(behind == uint64_t(kLanes - 1u - lane) * q * dlen, "lane %u: %llu bytes behind", lane,
          (unsigned long long)behind);
    out ^= advance(pow2, sq, behind, poly);
  }
  // by doubling: T(1) = c, T(2m) = T(m) * x0^m ^ T(m)
  uint32_t t = c, xm = x0;
  for (uint32_t m = 1; m < npk; m <<= 1) {
    t = mulmod(t, xm, poly) ^ t;
    xm = mulmod(xm, xm, poly);
  }
  CHECK(out == t, "2^39 bytes: by lanes %08x, by doubling %08x", out, t);
  CHECK(xm == zeros_op(1ull << 39, poly).apply(kOne) && xm == xpow8(pow2, 1ull << 39, poly), "x^(8 * 2^39)");
}

int main() {
  for (int ctype : {HDFS_CRC32C_CSUM_CRC32C, HDFS_CRC32C_CSUM_CRC32}) {
    const uint32_t poly = ctype == HDFS_CRC32C_CSUM_CRC32 ? hdfs_crc32c::kPolyZlib : hdfs_crc32c::kPoly;
    arithmetic(poly);
    streams(ctype, poly);
  }
  // the byte-wise CRC itself: "123456789"
  CHECK(ByteCrc(hdfs_crc32c::kPoly)(reinterpret_cast<const uint8_t *>("123456789"), 9) == 0xE3069283u, "CRC32C check");
  CHECK(ByteCrc(hdfs_crc32c::kPolyZlib)(reinterpret_cast<const uint8_t *>("123456789"), 9) == 0xCBF43926u, "CRC32 check");
  for (uint32_t poly : {hdfs_crc32c::kPoly, hdfs_crc32c::kPolyZlib}) {
    const ByteCrc crc(poly);
    std::vector<uint8_t> v(1031);
    fill(v);
    for (size_t n : {size_t(0), size_t(1), size_t(3), size_t(4), size_t(5), size_t(512), size_t(1031)})
      CHECK(crc(v.data(), n) == crc.bitwise(v.data(), n), "the reference CRC of %zu bytes", n);
  }
  std::printf("%llu checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
