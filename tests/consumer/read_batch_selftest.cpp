// Stand-alone check of the read batch library's probe arithmetic on the CPU:
// probe_entry, packet_of, record_of and prefix_regular (read_batch_layout.h),
// the functions probe_kernel runs with one thread per entry, against a
// brute-force frame::frame_step walk of the same stream.  Built with
// -fsanitize=address,undefined by tests/test_read_batch_cpu.py and run as a
// child process; nothing of it is loaded into Python.  A stream is allocated
// at exactly its length, so a read outside it is the sanitizer's to report.
// The streams are headers only: the data and CRC bytes are zeros, the layout
// does not look at them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "read_batch_layout.h"
#include "wire_fused_batch_lookup.h"

using namespace hdfs_read_batch;
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

// dlens in block order from offset 0, seqno from 7; sync: per packet.
static std::vector<Spec> specs(const std::vector<uint32_t> &dlens, bool empty_last, int sync = -1) {
  std::vector<Spec> v;
  int64_t off = 1 << 20;
  for (size_t k = 0; k < dlens.size(); k++) {
    v.push_back(Spec{dlens[k], off, int64_t(7 + k), !empty_last && k + 1 == dlens.size(), sync});
    off += dlens[k];
  }
  if (empty_last) v.push_back(Spec{0, off, int64_t(7 + dlens.size()), true, -1});
  return v;
}

static std::vector<uint8_t> build(int proto, const std::vector<Spec> &v) {
  uint64_t n = 0;
  for (const Spec &s : v) n += wire_bytes(proto, s);
  std::vector<uint8_t> out(n, 0);
  uint64_t pos = 0;
  for (const Spec &s : v) {
    put_header(out.data() + pos, proto, s);
    pos += wire_bytes(proto, s);
  }
  return out;
}

struct Walk {
  uint64_t npkts = 0, consumed = 0, delivered = 0;
  int error = 0;
};

// The walk of the main library's framing, one frame_step at a time; see(i, k)
// takes packet i's record.
template <class At, class See>
static Walk brute(At at, uint64_t len, int proto, uint32_t cs, int ctype, See see) {
  Walk w;
  uint64_t pos = 0;
  while (pos < len) {
    hdfs_crc32c_packet k;
    uint64_t total = 0;
    const int r = frame::frame_step(at(pos), len - pos, pos, proto, cs, ctype, k, total);
    if (r == frame::kStepMore) break;
    see(w.npkts++, k);
    if (k.error) {
      w.error = k.error;
      break;
    }
    pos += total;
    w.consumed = pos;
    w.delivered += uint64_t(k.data_len);
    if (r == frame::kStepStop) break;
  }
  return w;
}

struct Bytes {
  const uint8_t *s;
  const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

static bool same(const hdfs_crc32c_packet &a, const hdfs_crc32c_packet &b) {
  return a.stream_off == b.stream_off && a.offset_in_block == b.offset_in_block && a.seqno == b.seqno &&
         a.data_len == b.data_len && a.crc_len == b.crc_len && a.header_len == b.header_len && a.error == b.error &&
         a.first_bad == b.first_bad && a.bad_chunks == b.bad_chunks && a.last == b.last && a.sync == b.sync;
}

// probe_entry against the walk: the verdict, and for a regular stream every packet.
template <class At>
static Desc judge(const char *name, At at, uint64_t len, int proto, bool want_regular, uint64_t dst_cap = ~0ull,
                  bool records = true, uint64_t max_pkts = ~0ull, uint32_t cs = 512) {
  Desc d;
  std::memset(&d, 0xEE, sizeof(d));
  const bool regular = probe_entry(at, len, dst_cap, proto, cs, HDFS_CRC32C_CSUM_CRC32C, records, max_pkts, d);
  CHECK(regular == want_regular, "%s (proto %d): regular %d", name, proto, int(regular));
  if (!regular) {
    CHECK(d.npk == 0 && d.nbody == 0 && d.ntail == 0, "%s: an irregular entry has packets", name);
    return d;
  }
  uint64_t dst = 0;
  const Walk w = brute(at, len, proto, cs, HDFS_CRC32C_CSUM_CRC32C, [&](uint64_t i, const hdfs_crc32c_packet &k) {
    if (i >= d.npk) return;
    const PacketAt p = packet_of(d, uint32_t(i));
    CHECK(same(record_of(p), k), "%s: record %llu", name, (unsigned long long)i);
    CHECK(p.dst_off == dst, "%s: packet %llu goes to %llu, not %llu", name, (unsigned long long)i,
          (unsigned long long)p.dst_off, (unsigned long long)dst);
    CHECK(p.dlen <= kMaxData && p.stream_off + p.hb + 4ull * crc_count(p.dlen) + p.dlen <= d.consumed &&
              p.dst_off + p.dlen <= d.delivered,
          "%s: packet %llu leaves its ranges", name, (unsigned long long)i);
    dst += p.dlen;
  });
  CHECK(!w.error, "%s: the walk ends in error %d", name, w.error);
  CHECK(d.npk == w.npkts, "%s: %u packets, the walk has %llu", name, d.npk, (unsigned long long)w.npkts);
  CHECK(d.consumed == w.consumed && d.delivered == w.delivered, "%s: consumed %llu / %llu delivered %llu / %llu",
        name, (unsigned long long)d.consumed, (unsigned long long)w.consumed, (unsigned long long)d.delivered,
        (unsigned long long)w.delivered);
  CHECK(d.npk == d.nbody + d.ntail && d.ntail >= 1 && d.ntail <= kMaxTail, "%s: counts", name);
  CHECK(d.consumed <= len && d.delivered <= dst_cap, "%s: the bounds the kernel relies on", name);
  return d;
}

static void dense(const char *name, int proto, const std::vector<Spec> &v, bool want_regular, int64_t cut = 0,
                  uint64_t cap_short = 0, uint64_t max_pkts = ~0ull, uint32_t cs = 512) {
  const std::vector<uint8_t> all = build(proto, v);
  const uint64_t len = all.size() - uint64_t(cut);
  uint8_t *s = new uint8_t[len ? len : 1];  // exactly the stream
  std::memcpy(s, all.data(), len);
  uint64_t payload = 0;
  for (const Spec &x : v) payload += x.dlen;
  judge(name, Bytes{s}, len, proto, want_regular, cap_short ? payload - cap_short : ~0ull, true, max_pkts, cs);
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
  const std::vector<uint32_t> four = {65536, 65536, 65536, 12345};
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2}) {
    dense("[65536]*3 + [12345] + empty", proto, specs(four, true), true);
    dense("[512]", proto, specs({512}, false), true);
    dense("[512] + empty", proto, specs({512}, true), true);
    dense("[4096]*20", proto, specs(std::vector<uint32_t>(20, 4096), false), true);
    dense("[4096]*20 + empty", proto, specs(std::vector<uint32_t>(20, 4096), true), true);
    dense("[65536] + [700]", proto, specs({65536, 700}, false), true);
    dense("[512, 511] + empty (tail longer than a stride)", proto, specs({512, 511}, true), true);
    dense("only the empty last packet", proto, specs({}, true), false);
    dense("cut exactly after the run", proto, specs({65536, 65536, 65536}, false), true);
    dense("cut inside a header", proto, specs(four, true), true, 10);                  // the empty packet's
    dense("cut inside a data header", proto, specs({4096, 4096, 4096}, false), true, 4096 + 4 * 8 + 3);
    dense("cut inside the last packet's data", proto, specs(four, false), true, 100);  // the short packet is dropped
    dense("cut inside a full packet's data", proto, specs({8192, 8192, 8192}, false), true, 1);
    dense("a size break in the middle", proto, specs({65536, 65536, 4096, 65536, 65536}, false), false);
    dense("a longer packet behind the run", proto, specs({4096, 4096, 8192}, false), false);
    dense("two short packets", proto, specs({4096, 4096, 100, 100}, false), false);
    dense("[40000]*5", proto, specs(std::vector<uint32_t>(5, 40000), false), false);
    dense("dlen0 = 131072", proto, specs({131072, 131072}, true), false);
    dense("dlen0 = 256", proto, specs({256, 256}, true), false);
    dense("payload one byte more than dst_cap", proto, specs(four, true), false, 0, 1);
    dense("five packets, max_pkts 4", proto, specs(four, true), false, 0, 0, 4);
    dense("five packets, max_pkts 5", proto, specs(four, true), true, 0, 0, 5);
    dense("chunk_size 4096", proto, specs(std::vector<uint32_t>(3, 4096), true), false, 0, 0, ~0ull, 4096);
    {  // the last flag on the final full packet, nothing behind it
      std::vector<Spec> v = specs(std::vector<uint32_t>(6, 65536), false);
      dense("last on the final full packet", proto, v, true);
    }
    {  // an empty packet that is not the last one is a framing error
      std::vector<Spec> v = specs({4096, 4096}, true);
      v.back().last = false;
      dense("empty packet without the last flag", proto, v, false);
    }
  }
  // syncBlock (v2): on every packet, on the data packets alone, on one packet only
  {
    std::vector<Spec> v = specs(four, true, 1);
    dense("syncBlock on the data packets", 2, v, true);
    v.back().sync = 0;
    dense("syncBlock on every packet", 2, v, true);
    v = specs(std::vector<uint32_t>(6, 4096), true);
    v[3].sync = 1;
    dense("syncBlock on one packet only", 2, v, false);
    v = specs(std::vector<uint32_t>(6, 4096), false);
    v[5].sync = 1;
    dense("syncBlock on the last full packet only", 2, v, false);
  }
  // no records wanted: max_pkts is not looked at
  {
    const std::vector<uint8_t> s = build(2, specs(four, true));
    judge("no records wanted", Bytes{s.data()}, s.size(), 2, true, ~0ull, false, 0);
  }
  // 2^39 bytes: the 64-bit offsets
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2}) {
    Sparse sp;
    sp.proto = proto;
    sp.dlen = 65536;
    sp.tail_dlen = 1000;
    sp.stride = wire_bytes(proto, Spec{65536, 0, 0, false, -1});
    const uint64_t len = 1ull << 39;
    const uint64_t tail = wire_bytes(proto, Spec{1000, 0, 0, false, -1}) + wire_bytes(proto, Spec{0, 0, 0, true, -1});
    sp.K = (len - tail) / sp.stride;
    const uint64_t exact = sp.K * sp.stride + tail;  // a few slack bytes behind the empty packet are not consumed
    const Desc d = judge("2^39 bytes", sp, len, proto, true);
    CHECK(d.consumed == exact && d.consumed > (1ull << 38) && d.nbody == sp.K - 1 && d.ntail == 3,
          "2^39 bytes: consumed %llu", (unsigned long long)d.consumed);
    const PacketAt p = packet_of(d, d.nbody - 1u);
    CHECK(p.stream_off == (sp.K - 2) * sp.stride && p.stream_off > (1ull << 38) && p.dst_off == (sp.K - 2) * 65536ull,
          "2^39 bytes: the last body packet");
  }
  // the prefix array and the lookup over a batch that mixes regular and irregular entries
  {
    const uint32_t npk[] = {0, 5, 0, 0, 1, 2049, 0, 1, 1, 0};
    const uint32_t n = sizeof(npk) / sizeof(npk[0]);
    uint32_t *slot = new uint32_t[n], *pk0 = new uint32_t[n + 1];
    const uint32_t nreg = prefix_regular(npk, n, slot, pk0);
    CHECK(nreg == 5 && pk0[nreg] == 5 + 1 + 2049 + 1 + 1, "prefix: %u regular, %u packets", nreg, pk0[nreg]);
    uint32_t s = 0, total = 0;
    for (uint32_t e = 0; e < n; e++) {
      if (!npk[e]) {
        CHECK(slot[e] == kNoSlot, "prefix: irregular entry %u has a slot", e);
        continue;
      }
      CHECK(slot[e] == s && pk0[s] == total, "prefix: entry %u", e);
      for (uint32_t g = total; g < total + npk[e]; g++)
        for (uint32_t hint = 0; hint <= s; hint++)
          CHECK(hdfs_wire_fused::write_of(pk0, nreg, g, hint) == s, "write_of(%u, hint %u)", g, hint);
      total += npk[e];
      s++;
    }
    // an entry that would take the launch past its packet limit is left out
    const uint32_t big[] = {kMaxPackets - 1u, 2, 1};
    CHECK(prefix_regular(big, 3, slot, pk0) == 2 && slot[1] == kNoSlot && slot[2] == 1 && pk0[2] == kMaxPackets,
          "prefix: the packet limit");
    const uint32_t none[] = {0, 0};
    CHECK(prefix_regular(none, 2, slot, pk0) == 0 && pk0[0] == 0, "prefix: no regular entry");
    delete[] slot;
    delete[] pk0;
  }
  std::printf("%llu checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
