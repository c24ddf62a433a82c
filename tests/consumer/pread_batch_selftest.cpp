// Stand-alone check of the pread batch library's window arithmetic on the CPU:
// probe_window and place_of (pread_batch_layout.h) with packet_of and
// record_of (read_batch_layout.h), the functions pread_probe_kernel runs with
// one thread per entry, against a brute-force walk of the same stream:
// frame::frame_step per packet with frame::read_avail and the read loop's stop
// rules (src/datanode.c:1476-1481, 2478-2549).  Built with
// -fsanitize=address,undefined by tests/test_pread_batch_cpu.py and run as a
// child process; nothing of it is loaded into Python.  A stream is allocated
// at exactly its length, so a read outside it is the sanitizer's to report.
// The streams are headers only: the data and CRC bytes are zeros, the layout
// does not look at them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "pread_batch_layout.h"

using namespace hdfs_pread_batch;
namespace frame = hdfs_crc32c::frame;

static int failures = 0;
static unsigned long long checks = 0, regulars = 0, irregulars = 0;
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
  be(p + 4, 25, 2);
  uint8_t *q = p + 6;
  q[0] = 0x09;
  le(q + 1, uint64_t(s.off), 8);
  q[9] = 0x11;
  le(q + 10, uint64_t(s.seq), 8);
  q[18] = 0x18;
  q[19] = s.last ? 1 : 0;
  q[20] = 0x25;
  le(q + 21, s.dlen, 4);
  return 31;
}

static uint64_t wire_bytes(int proto, const Spec &s) {
  return (proto == HDFS_CRC32C_PROTO_V1 ? 25u : 31u) + 4ull * ((s.dlen + 511u) / 512u) + s.dlen;
}

// K packets of dlen0, a shorter one (0: none), the empty last one or the last
// flag on the final data packet; offsets from offset0, seqno from 7.
static std::vector<Spec> specs(uint32_t dlen0, uint32_t K, uint32_t shorter, bool empty_last, int64_t offset0) {
  std::vector<Spec> v;
  int64_t off = offset0;
  const uint32_t n = K + (shorter ? 1u : 0u);
  for (uint32_t k = 0; k < n; k++) {
    const uint32_t dl = k < K ? dlen0 : shorter;
    v.push_back(Spec{dl, off, int64_t(7 + k), !empty_last && k + 1 == n});
    off += dl;
  }
  if (empty_last) v.push_back(Spec{0, off, int64_t(7 + n), true});
  return v;
}

// The stream, allocated at exactly its length.
struct Stream {
  uint8_t *s;
  uint64_t len;
  Stream(int proto, const std::vector<Spec> &v, uint64_t cut = 0) {
    uint64_t n = 0;
    for (const Spec &x : v) n += x.dlen ? wire_bytes(proto, x) : (proto == HDFS_CRC32C_PROTO_V1 ? 25u : 31u);
    std::vector<uint8_t> all(n, 0);
    uint64_t pos = 0;
    for (const Spec &x : v) {
      put_header(all.data() + pos, proto, x);
      pos += x.dlen ? wire_bytes(proto, x) : (proto == HDFS_CRC32C_PROTO_V1 ? 25u : 31u);
    }
    len = n - cut;
    s = new uint8_t[len ? len : 1];
    std::memcpy(s, all.data(), len);
  }
  ~Stream() { delete[] s; }
  Stream(const Stream &) = delete;
};

struct Bytes {
  const uint8_t *s;
  const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

struct Take {
  hdfs_crc32c_packet rec;
  uint64_t dst_off;
  uint32_t c_begin, n;
};

struct Walk {
  std::vector<Take> takes;
  uint64_t npkts = 0, consumed = 0, delivered = 0;
  int rc = 0;
  bool complete = false;  // a clean read of every byte wanted
};

// The read loop of hdfs_crc32c_read_packets with a destination of read_len
// bytes and room for max_pkts records.
static Walk brute(const Stream &st, int proto, int64_t client_offset, int64_t read_len, uint64_t max_pkts) {
  Walk w;
  if (client_offset < 0 || read_len <= 0) {
    w.rc = HDFS_CRC32C_EINVAL;
    return w;
  }
  uint64_t pos = 0, remains = uint64_t(read_len);
  while (pos < st.len && remains && w.npkts < max_pkts) {
    hdfs_crc32c_packet k;
    uint64_t total = 0;
    const int r = frame::frame_step(st.s + pos, st.len - pos, pos, proto, 512, HDFS_CRC32C_CSUM_CRC32C, k, total);
    if (r == frame::kStepMore) break;  // incomplete: the walk ends ahead of it, the read is short
    w.npkts++;
    if (k.error) {
      w.rc = k.error;
      break;
    }
    if (r == frame::kStepStop) {  // the empty last packet before the read is complete
      w.consumed = pos + total;
      w.rc = HDFS_CRC32C_ERR_DATANODE_BAD_LASTPACKET;
      break;
    }
    uint32_t cb = 0;
    const uint32_t avail = frame::read_avail(k, true, client_offset, cb);
    if (!avail) {
      w.rc = HDFS_CRC32C_ERR_DATANODE_UNEXPECTED_READ_OFFSET;
      break;
    }
    const uint32_t n = uint32_t(avail < remains ? avail : remains);
    w.takes.push_back(Take{k, w.delivered, cb, n});
    w.delivered += n;
    remains -= n;
    pos += total;
    w.consumed = pos;
    if (k.last && remains) {
      w.rc = HDFS_CRC32C_ERR_DATANODE_BAD_LASTPACKET;
      break;
    }
  }
  w.complete = !w.rc && !remains;
  return w;
}

static bool same(const hdfs_crc32c_packet &a, const hdfs_crc32c_packet &b) {
  return a.stream_off == b.stream_off && a.offset_in_block == b.offset_in_block && a.seqno == b.seqno &&
         a.data_len == b.data_len && a.crc_len == b.crc_len && a.header_len == b.header_len && a.error == b.error &&
         a.first_bad == b.first_bad && a.bad_chunks == b.bad_chunks && a.last == b.last && a.sync == b.sync;
}

// probe_window against the walk.  -> the verdict.
static bool judge(const char *name, const Stream &st, int proto, int64_t client_offset, int64_t read_len,
                  uint64_t dst_cap, bool records = true, uint64_t max_pkts = ~0ull, bool in_sequence = true) {
  Window w;
  std::memset(&w, 0xEE, sizeof(w));
  const bool regular = probe_window(Bytes{st.s}, st.len, dst_cap, client_offset, read_len, proto, 512,
                                    HDFS_CRC32C_CSUM_CRC32C, records, max_pkts, w);
  const Walk b = brute(st, proto, client_offset, read_len, records ? max_pkts : ~0ull);
  const bool fits = read_len > 0 && uint64_t(read_len) <= dst_cap;
  hdfs_read_batch::Desc shape;
  const bool shaped = probe_entry(Bytes{st.s}, st.len, ~0ull, proto, 512, HDFS_CRC32C_CSUM_CRC32C, false, 0, shape);
#define WHERE "%s (proto %d, offset %lld, length %lld)", name, proto, (long long)client_offset, (long long)read_len
  if (!b.complete || !fits) CHECK(!regular, WHERE);
  if (b.complete && fits && shaped && in_sequence) CHECK(regular, WHERE);
  if (!regular) {
    irregulars++;
    CHECK(w.d.npk == 0 && w.d.nbody == 0 && w.d.ntail == 0 && w.d.consumed == 0 && w.d.delivered == 0 &&
              w.c_begin == 0 && w.w_end == 0, WHERE);
    return false;
  }
  regulars++;
  const Desc &d = w.d;
  CHECK(b.complete && fits, WHERE);
  CHECK(d.npk == b.npkts && d.npk == b.takes.size() && d.npk == d.nbody + d.ntail && d.ntail <= kMaxTail, WHERE);
  CHECK(d.consumed == b.consumed && d.consumed <= st.len, WHERE);
  CHECK(d.delivered == b.delivered && d.delivered == uint64_t(read_len) && w.w_end - w.c_begin == d.delivered, WHERE);
  CHECK(!b.takes.empty() && w.c_begin == b.takes[0].c_begin, WHERE);
  for (uint32_t i = 0; i < d.npk && i < b.takes.size(); i++) {
    const PacketAt p = packet_of(d, i);
    const Take &t = b.takes[i];
    uint32_t from = 0, n = 0;
    uint64_t at = 0;
    place_of(w, p, from, at, n);
    CHECK(same(record_of(p), t.rec), WHERE);
    CHECK(from == t.c_begin && at == t.dst_off && n == t.n, WHERE);
    // the bounds the kernel relies on
    CHECK(p.stream_off + p.hb + 4ull * hdfs_read_batch::crc_count(p.dlen) + p.dlen <= d.consumed &&
              at + n <= uint64_t(read_len) && from + n <= p.dlen && n > 0, WHERE);
  }
#undef WHERE
  return true;
}

int main() {
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2})
    for (const uint32_t dlen0 : {512u, 4096u, 65536u})
      for (const uint32_t K : {1u, 2u, 3u, 5u})
        for (const uint32_t shorter : {0u, 1u, 511u, 512u, 700u})
          for (const bool empty_last : {true, false})
            for (const int64_t offset0 : {int64_t(0), int64_t(512), int64_t(1) << 20}) {
              const Stream st(proto, specs(dlen0, K, shorter, empty_last, offset0));
              const uint64_t payload = uint64_t(K) * dlen0 + shorter;
              for (const int64_t diff : {int64_t(-5), int64_t(0), int64_t(1), int64_t(511), int64_t(512),
                                         int64_t(dlen0) - 1, int64_t(dlen0)}) {
                const int64_t client_offset = offset0 + diff;
                const uint64_t cb = diff > 0 ? uint64_t(diff) : 0u;
                const uint64_t ragged0 = uint64_t(K) * dlen0 + shorter / 512u * 512u;
                // the read's end, in payload positions
                const uint64_t ends[] = {cb + 1u,                              // one byte in
                                         (cb + 16u) / 16u * 16u,               // at a 16-B boundary
                                         (cb + 16u) / 16u * 16u + 7u,          // mid-piece
                                         (cb + 4096u) / 4096u * 4096u,         // at a round boundary
                                         dlen0,                                // at a packet boundary
                                         uint64_t(K) * dlen0,                  // at the last full packet's end
                                         ragged0 + 1u,                         // inside the ragged chunk (when there is one)
                                         payload - 1u, payload, payload + 1u};  // around the payload's end
                for (const uint64_t end : ends) {
                  if (end <= cb) continue;
                  const int64_t read_len = int64_t(end - cb);
                  const bool reg = judge("matrix", st, proto, client_offset, read_len, uint64_t(read_len));
                  if (reg) {  // the destination one byte short (AGAIN), the records one short, no records wanted
                    judge("dst_cap = read_len - 1", st, proto, client_offset, read_len, uint64_t(read_len) - 1u);
                    Window w;
                    probe_window(Bytes{st.s}, st.len, ~0ull, client_offset, read_len, proto, 512,
                                 HDFS_CRC32C_CSUM_CRC32C, false, 0, w);
                    judge("max_pkts one short", st, proto, client_offset, read_len, ~0ull, true, w.d.npk - 1u);
                    judge("max_pkts exact", st, proto, client_offset, read_len, ~0ull, true, w.d.npk);
                    CHECK(judge("no records wanted", st, proto, client_offset, read_len, ~0ull, false, 0), "no records");
                  }
                }
              }
            }
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2}) {
    // the last flag on packet 0 of three: a read inside packet 0 is served, a longer one is BAD_LASTPACKET
    std::vector<Spec> v = specs(4096, 3, 700, true, 1 << 20);
    v[0].last = true;
    {
      const Stream st(proto, v);
      CHECK(judge("last on packet 0, read inside it", st, proto, (1 << 20) + 100, 3996, 3996), "served");
      CHECK(!judge("last on packet 0, read past it", st, proto, (1 << 20) + 100, 3997, 3997), "refused");
    }
    // the last flag on packet K - 1 ahead of the shorter packet
    v = specs(4096, 3, 700, true, 0);
    v[2].last = true;
    {
      const Stream st(proto, v);
      CHECK(judge("last on packet K - 1, read ends in it", st, proto, 10, 3 * 4096 - 10, 1 << 20), "served");
      CHECK(!judge("last on packet K - 1, read goes on", st, proto, 10, 3 * 4096 - 9, 1 << 20), "refused");
    }
    // a stream cut inside a packet: reads that end ahead of the cut are served
    {
      const Stream st(proto, specs(65536, 3, 0, false, 0), 1000);
      CHECK(judge("cut stream, read inside packet 1", st, proto, 300, 2 * 65536 - 300, 1 << 20), "served");
      CHECK(!judge("cut stream, read into the cut packet", st, proto, 300, 2 * 65536 - 299, 1 << 20), "refused");
    }
    // An offsetInBlock off the sequence on a packet the probe takes as framed (packet K - 1, the shorter
    // one): the main library applies read_avail to that packet's own offset, so the entry is not the
    // kernel's whenever the packet is taken -- whether the walk then ends in UNEXPECTED_READ_OFFSET, skips
    // bytes of it, or delivers the same bytes -- and is unaffected when the read ends ahead of it.
    for (const int which : {0, 1})        // packet K - 1, the shorter packet
      for (const int64_t to : {int64_t(0), int64_t(1 << 20) + 50, int64_t(1 << 20) + 4096 * 3 - 512,
                               int64_t(1 << 20) + 4096 * 3 + 512, int64_t(1) << 40}) {
        std::vector<Spec> o = specs(4096, 3, 700, true, 1 << 20);
        const size_t at = which ? 3 : 2;
        if (o[at].off == to) continue;
        o[at].off = to;
        const Stream st(proto, o);
        const int64_t c0 = (1 << 20) + 100;
        judge("off-sequence tail, read ends ahead of it", st, proto, c0, int64_t(at) * 4096 - 100, 1 << 20);
        CHECK(!judge("off-sequence tail, read ends inside it", st, proto, c0, int64_t(at) * 4096 - 100 + 10, 1 << 20,
                     true, ~0ull, false),
              "packet %zu at offset %lld must not be the kernel's", at, (long long)to);
        CHECK(!judge("off-sequence tail, read to the payload's end", st, proto, c0, 3 * 4096 + 700 - 100, 1 << 20, true,
                     ~0ull, false),
              "packet %zu at offset %lld must not be the kernel's", at, (long long)to);
      }
    {  // the reviewer's stream: two 4 KiB packets at 1 MiB, packet 1 naming offset 0
      std::vector<Spec> o = specs(4096, 2, 0, true, 1 << 20);
      o[1].off = 0;
      const Stream st(proto, o);
      const Walk b = brute(st, proto, (1 << 20) + 100, 6000, ~0ull);
      CHECK(b.rc == HDFS_CRC32C_ERR_DATANODE_UNEXPECTED_READ_OFFSET && b.delivered == 3996, "the walk: rc %d", b.rc);
      CHECK(!judge("packet 1 names offset 0", st, proto, (1 << 20) + 100, 6000, 6000, true, ~0ull, false), "refused");
      CHECK(judge("packet 1 names offset 0, read inside packet 0", st, proto, (1 << 20) + 100, 3996, 3996), "served");
    }
    {  // a shorter packet 50 bytes below the read's start: rc 0 on the walk, 50 bytes of it skipped
      std::vector<Spec> o = specs(4096, 1, 700, true, 1 << 20);
      o[1].off = (1 << 20) + 100 - 50;
      const Stream st(proto, o);
      const Walk b = brute(st, proto, (1 << 20) + 100, 4200, ~0ull);
      CHECK(b.complete && b.takes.size() == 2 && b.takes[1].c_begin == 50, "the walk skips 50 bytes");
      CHECK(!judge("shorter packet below the read's start", st, proto, (1 << 20) + 100, 4200, 4200, true, ~0ull, false),
            "refused");
    }
    // read_len <= 0 and READ_ALL are never regular
    {
      const Stream st(proto, specs(4096, 2, 0, true, 0));
      Window w;
      for (const int64_t rl : {int64_t(0), int64_t(-1), int64_t(-7)})
        CHECK(!probe_window(Bytes{st.s}, st.len, ~0ull, 0, rl, proto, 512, HDFS_CRC32C_CSUM_CRC32C, false, 0, w) &&
                  w.d.npk == 0, "read_len %lld", (long long)rl);
      CHECK(!probe_window(Bytes{st.s}, st.len, ~0ull, 0, 100, proto, 4096, HDFS_CRC32C_CSUM_CRC32C, false, 0, w),
            "chunk_size 4096");
    }
  }
  std::printf("%llu regular, %llu irregular verdicts\n%llu checks\n%d failures\n", regulars, irregulars, checks,
              failures);
  return failures || !regulars || !irregulars ? 1 : 0;
}
