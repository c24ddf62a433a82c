// Stand-alone check of the relay batch library's own arithmetic on the CPU:
// relay_batch_lookup.h (out_shape, seek, next_chunk, data_at, crc_at,
// first_header, end_header) and relay_batch_internal.h's geom_of, the functions
// the probe and relay_fused_batch_kernel run, against a per-byte model: a
// frame::frame_step walk of the input stream says where every payload byte and
// every chunk's CRC word lie, outpkt::plan_out_packets says what the write's
// stream is.  Built with -fsanitize=address,undefined by
// tests/test_relay_batch_cpu.py and run as a child process; nothing of it is
// loaded into Python.  The streams are headers only: the data and CRC bytes are
// zeros, the arithmetic does not look at them.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "crc32c_outpkt.h"
#include "read_batch_layout.h"
#include "relay_batch_internal.h"
#include "relay_batch_lookup.h"
#include "wire_internal.h"

using namespace hdfs_relay_batch;
namespace frame = hdfs_crc32c::frame;
namespace outpkt = hdfs_crc32c::outpkt;

static int failures = 0;
static unsigned long long checks = 0;
#define CHECK(c, ...)                                           \
  do {                                                          \
    checks++;                                                   \
    if (!(c)) {                                                 \
      if (++failures < 30) {                                    \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c); \
        std::printf(__VA_ARGS__);                               \
        std::printf("\n");                                      \
      }                                                         \
    }                                                           \
  } while (0)

static void be(uint8_t *p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = uint8_t(v >> (8 * (n - 1 - i)));
}
static void le(uint8_t *p, uint64_t v, int n) {
  for (int i = 0; i < n; i++) p[i] = uint8_t(v >> (8 * i));
}

// A packet's header bytes, written out by hand.  -> their count.
static uint32_t put_header(uint8_t *p, int proto, uint32_t dlen, int64_t off, int64_t seq, bool last) {
  const uint32_t ncrc = (dlen + 511u) / 512u;
  be(p, dlen + 4u * ncrc + 4u, 4);
  if (proto == HDFS_CRC32C_PROTO_V1) {
    be(p + 4, uint64_t(off), 8);
    be(p + 12, uint64_t(seq), 8);
    p[20] = last ? 1 : 0;
    be(p + 21, dlen, 4);
    return 25;
  }
  be(p + 4, 25, 2);
  uint8_t *q = p + 6;
  q[0] = 0x09;
  le(q + 1, uint64_t(off), 8);
  q[9] = 0x11;
  le(q + 10, uint64_t(seq), 8);
  q[18] = 0x18;
  q[19] = last ? 1 : 0;
  q[20] = 0x25;
  le(q + 21, dlen, 4);
  return 31;
}

static std::vector<uint8_t> build(int proto, const std::vector<uint32_t> &dlens, bool empty_last) {
  std::vector<uint8_t> out;
  int64_t off = 1 << 20, seq = 7;
  auto put = [&](uint32_t dlen, bool last) {
    uint8_t h[40];
    const uint32_t hb = put_header(h, proto, dlen, off, seq++, last);
    out.insert(out.end(), h, h + hb);
    out.resize(out.size() + 4u * ((dlen + 511u) / 512u) + dlen, 0);
    off += dlen;
  };
  for (size_t k = 0; k < dlens.size(); k++) put(dlens[k], !empty_last && k + 1 == dlens.size());
  if (empty_last) put(0, true);
  return out;
}

struct Bytes {
  const uint8_t *s;
  const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

// The walk's model of a stream.
struct Model {
  std::vector<uint32_t> src;      // payload byte y lies at stream offset src[y]
  std::vector<uint32_t> crc;      // payload chunk q's CRC word lies at stream offset crc[q]
  std::vector<uint64_t> first;    // packet i's first data byte in the payload (the empty packet: the payload's end)
  uint64_t consumed = 0;
};

static Model walk(const std::vector<uint8_t> &s, int proto) {
  Model m;
  uint64_t pos = 0;
  while (pos < s.size()) {
    hdfs_crc32c_packet k;
    uint64_t total = 0;
    const int r = frame::frame_step(s.data() + pos, s.size() - pos, pos, proto, 512, HDFS_CRC32C_CSUM_CRC32C, k, total);
    if (r == frame::kStepMore || k.error) break;
    m.first.push_back(m.src.size());
    const uint64_t c0 = k.stream_off + k.header_len, d0 = c0 + uint64_t(k.crc_len);
    for (int32_t b = 0; b < k.data_len; b++) m.src.push_back(uint32_t(d0 + uint64_t(b)));
    for (int32_t c = 0; c < k.crc_len / 4; c++) m.crc.push_back(uint32_t(c0 + 4u * uint64_t(c)));
    pos += total;
    m.consumed = pos;
    if (r == frame::kStepStop) break;
  }
  return m;
}

// ---- the closed form of an aligned write's stream against its plan ------------------------------
static void shape(uint64_t payload) {
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2})
    for (const int64_t off : {int64_t(0), int64_t(512), int64_t(3584), (int64_t(1) << 31) + 512})
      for (const bool finish : {false, true}) {
        std::vector<outpkt::OutPlan> plan;
        outpkt::plan_out_packets(payload, off, 3, finish, plan);
        uint64_t wire_len = 0, npk = 0;
        out_shape(payload, outpkt::out_header_bytes(proto), finish, wire_len, npk);
        CHECK(npk == plan.size() && wire_len == outpkt::out_plan_bytes(plan, proto, true) + payload,
              "out_shape(%llu, proto %d, off %lld, finish %d): %llu bytes in %llu packets", (unsigned long long)payload,
              proto, (long long)off, int(finish), (unsigned long long)wire_len, (unsigned long long)npk);
      }
}

// ---- one stream ------------------------------------------------------------------------------------
static void relay(const char *name, int proto, const std::vector<uint32_t> &dlens, bool empty_last) {
  const std::vector<uint8_t> all = build(proto, dlens, empty_last);
  uint8_t *s = new uint8_t[all.size()];  // exactly the stream
  std::memcpy(s, all.data(), all.size());
  const Model m = walk(all, proto);
  hdfs_read_batch::Desc d;
  const bool regular = hdfs_read_batch::probe_entry(Bytes{s}, all.size(), ~0ull, proto, 512, HDFS_CRC32C_CSUM_CRC32C,
                                                    false, 0, d);
  delete[] s;
  CHECK(regular, "%s (proto %d): not regular", name, proto);
  if (!regular) return;
  const Geom g = geom_of(d);
  const uint64_t P = m.src.size();
  CHECK(g.payload == P && d.consumed == m.consumed && in_packets(g) == d.npk && d.npk == m.first.size() &&
            d.consumed < kMaxConsumed,
        "%s (proto %d): payload %llu, %u packets", name, proto, (unsigned long long)g.payload, in_packets(g));
  shape(P);
  const uint32_t hb = outpkt::out_header_bytes(proto);
  for (const bool finish : {false, true}) {
    uint64_t wire_len = 0, npk = 0;
    out_shape(P, hb, finish, wire_len, npk);
    const hdfs_wire::Write w{nullptr, nullptr, nullptr, P, 3584, 3, 0u, uint32_t(npk), hb, uint32_t(proto), 1u,
                             finish ? 1u : 0u, 0u};
    std::vector<uint8_t> covered(P, 0), seen(d.npk, 0);
    uint64_t at = 0;
    for (uint32_t j = 0; j < npk; j++) {
      const hdfs_wire::Pkt p = hdfs_wire::packet_at(w, j);
      // the output side: the packets tile [0, wire_len)
      const uint64_t y0 = uint64_t(j) * kOutData < P ? uint64_t(j) * kOutData : P;  // the empty last packet: the end
      CHECK(p.wire_off == at && p.data_off == y0, "%s: output packet %u lies at %llu", name, j,
            (unsigned long long)p.wire_off);
      at += hb + 4ull * p.ncrc + p.dlen;
      CHECK(at <= wire_len && p.data_off + p.dlen <= P, "%s: output packet %u leaves the stream", name, j);
      // the rounds: wave v's eight chunks, each from its place in the input
      const uint32_t nfull = p.dlen / kGrid, n = p.dlen % kGrid;
      for (uint32_t v = 0; v < 16; v++) {
        const uint32_t first = 8u * v;
        const uint32_t nfr = nfull > first ? (nfull - first < 8u ? nfull - first : 8u) : 0u;
        Cursor c = seek(g, j * kOutChunks + first);
        for (uint32_t i = 0; i < 8; i++, c = next_chunk(g, c)) {
          if (i >= nfr) continue;
          const uint64_t y = p.data_off + 4096ull * v + 512ull * i, da = data_at(g, c), ca = crc_at(g, c);
          CHECK(da + kGrid <= d.consumed && ca + 4u <= d.consumed, "%s: chunk at payload %llu leaves the stream", name,
                (unsigned long long)y);
          CHECK(ca == m.crc[y / kGrid], "%s: CRC word of payload chunk %llu at %llu, the walk has %u", name,
                (unsigned long long)(y / kGrid), (unsigned long long)ca, m.crc[y / kGrid]);
          bool same = true;
          for (uint32_t b = 0; b < kGrid; b++) {
            same = same && da + b == m.src[y + b];
            covered[y + b]++;
          }
          CHECK(same, "%s: payload chunk at %llu comes from %llu, the walk has %u", name, (unsigned long long)y,
                (unsigned long long)da, m.src[y]);
        }
      }
      if (n) {  // the ragged chunk behind the packet's full ones
        const Cursor c = seek(g, uint32_t(g.payload / kGrid));
        const uint64_t y = p.data_off + uint64_t(kGrid) * nfull, da = data_at(g, c), ca = crc_at(g, c);
        CHECK(y / kGrid == P / kGrid && y + n == P, "%s: a ragged chunk ahead of the payload's end", name);
        CHECK(da + n <= d.consumed && ca == m.crc[y / kGrid], "%s: the ragged chunk's places", name);
        for (uint32_t b = 0; b < n; b++) {
          CHECK(da + b == m.src[y + b], "%s: ragged byte %u", name, b);
          covered[y + b]++;
        }
      }
      // the input headers this output packet's workgroup compares
      const uint32_t h0 = first_header(g, j), h1 = end_header(g, j, uint32_t(npk));
      CHECK(h0 <= h1 && h1 <= d.npk, "%s: headers [%u, %u) of output packet %u", name, h0, h1, j);
      for (uint32_t i = h0; i < h1 && i < d.npk; i++) {
        seen[i]++;
        const bool data = i < in_data_packets(g);
        CHECK(data ? m.first[i] / kOutData == j : j + 1u == npk, "%s: input header %u is compared by output packet %u",
              name, i, j);
        const hdfs_read_batch::PacketAt pa = hdfs_read_batch::packet_of(d, i);
        CHECK(pa.stream_off + pa.hb <= d.consumed && (data ? pa.dlen != 0u : pa.dlen == 0u), "%s: input packet %u", name,
              i);
      }
    }
    CHECK(at == wire_len, "%s: the output packets end at %llu of %llu", name, (unsigned long long)at,
          (unsigned long long)wire_len);
    bool once = true;
    for (uint64_t y = 0; y < P; y++) once = once && covered[y] == 1;
    CHECK(once, "%s: a payload byte is not stored exactly once", name);
    for (uint32_t i = 0; i < d.npk; i++)
      CHECK(seen[i] == 1, "%s (finish %d): input header %u is compared %u times", name, int(finish), i, seen[i]);
  }
}

int main() {
  for (const int proto : {HDFS_CRC32C_PROTO_V1, HDFS_CRC32C_PROTO_V2})
    for (const uint32_t dlen0 : {512u, 1024u, 4096u, 5120u, 64512u, 65536u})
      for (const uint32_t K : {1u, 2u, 3u, 5u, 130u})
        for (const uint32_t shorter : {0u, 1u, 511u, 512u, 700u})
          for (const bool empty_last : {false, true}) {
            if (shorter >= dlen0) continue;  // not a shorter packet
            std::vector<uint32_t> dlens(K, dlen0);
            if (shorter) dlens.push_back(shorter);
            char name[96];
            std::snprintf(name, sizeof(name), "[%u]*%u + [%u]%s", dlen0, K, shorter, empty_last ? " + empty" : "");
            relay(name, proto, dlens, empty_last);
          }
  // sizes of the write alone, across the 4 GiB a payload of the kernel stays below
  for (const uint64_t payload : {0ull, 1ull, 511ull, 512ull, 513ull, 65535ull, 65536ull, 65537ull, 131072ull,
                                 (8ull << 20) + 777ull})
    shape(payload);
  std::printf("%llu checks\n%d failures\n", checks, failures);
  return failures ? 1 : 0;
}
