// libhadoofus_md5crc_streams.so: entry points of
// include/hadoofus_md5crc_streams.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Its kernels (md5crc_streams_kernels.hip) frame the regular entries of a
// batch, check their headers and digest their CRC regions where they lie.
// Every other entry is framed by hdfs_crc32c_parse_packets, called here after
// the synchronise: this file holds no walk of its own.  The CRC regions that
// walk records are gathered in the library's scratch and digested by the same
// kernel through a descriptor of one region.  The run, the walk in pieces and
// the collection of the entries' outcomes are read_batch_host.h's.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "companion_support.h"
#include "hadoofus_md5crc_streams.h"
#include "md5_core.h"
#include "md5crc_streams_internal.h"
#include "md5crc_streams_lookup.h"
#include "read_batch_host.h"
#include "read_batch_layout.h"

namespace hdfs_md5crc_streams {
namespace {

using namespace hdfs_companion;

static_assert(HDFS_MD5CRC_STREAMS_MAX_ENTRIES == kMaxEntries, "the header's limit is the probe's");
static_assert(sizeof(hdfs_md5crc_streams_entry) == 80, "the ABI of version 1");

// ---- device state -------------------------------------------------------------
// On the engine's device: the call's device tables and their pinned twin, and
// the fallback's scratch (descriptors, digests, the gather's records and the
// gathered CRCs), all grown on demand, never shrunk, kept between calls.  Calls
// hold g_mu from the tables' upload to the last fallback entry, so one call's
// tables are never overwritten under its kernels or under the host's reading
// of them.
std::mutex g_mu;
struct Scratch : DeviceScratch {
  TablePair tab;
  DeviceBuffer gather;
  std::vector<hdfs_crc32c_packet> recs;  // a fallback entry's records, a piece of the walk at a time

  int reserve(int to, size_t tab_bytes) {
    const int rc = bind(to, "stream", [this] {
      tab.release();
      gather.release();
    });
    return rc ? rc : tab.reserve(tab_bytes, kTableFloor);
  }
} g_s;

void clear_outputs(hdfs_md5crc_streams_entry *e, size_t n) {
  for (size_t b = 0; b < n; b++) {
    e[b].consumed = e[b].payload = e[b].nchunks = e[b].npkts = 0;
    e[b].offset_in_block = 0;
    e[b].rc = 0;
    e[b].path = HDFS_MD5CRC_STREAMS_PATH_KERNEL;
    std::memset(e[b].md5, 0, sizeof(e[b].md5));
  }
}

// ---- argument checks that need no device ------------------------------------------
int check_arguments(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype) {
  if (!e || !n) return fail(HDFS_CRC32C_EINVAL, "entry 0: no entries");
  if (n > kMaxEntries)
    return fail(HDFS_CRC32C_EINVAL, "entry %u: %zu entries, at most %u in one call", unsigned(kMaxEntries), n,
                unsigned(kMaxEntries));
  clear_outputs(e, n);
  if (!packet_args_ok(proto, ctype, 0)) return prefix_fail(HDFS_CRC32C_EINVAL, "entry 0");
  if (ctype == HDFS_CRC32C_CSUM_NULL)
    return fail(HDFS_CRC32C_EINVAL, "entry 0: no CRCs to digest without CRC32 or CRC32C");
  if (!chunk_size) return fail(HDFS_CRC32C_EINVAL, "entry 0: chunk_size 0");
  for (size_t b = 0; b < n; b++)
    if (e[b].len && !e[b].stream) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null stream", b);
  return HDFS_CRC32C_OK;
}

// ---- MD5 on the host (md5_core.h's rounds) ----------------------------------------------
void state_bytes(const uint32_t st[4], uint8_t out[16]) {
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 4; k++) out[4 * j + k] = uint8_t(st[j] >> (8 * k));
}

// MD5 of nwords little-endian words: block_words' padding, the kernel's length words.
void md5_of_words(const uint32_t *w, uint64_t nwords, uint8_t out[16]) {
  using namespace hdfs_md5crc;
  uint32_t st[4];
  md5_init(st);
  const uint64_t nblk = md5_words_blocks(nwords);
  for (uint64_t b = 0; b < nblk; b++) {
    uint32_t m[16];
    for (uint32_t j = 0; j < 16; j++) {
      const uint64_t i = 16 * b + j;
      m[j] = i < nwords ? w[i] : i == nwords ? 0x00000080u : 0u;
    }
    if (b + 1 == nblk) {
      m[14] = uint32_t(nwords << 5);
      m[15] = uint32_t(nwords >> 27);
    }
    md5_block(st, m);
  }
  state_bytes(st, out);
}

// ---- an entry handed to the main library ------------------------------------------------
// What the fallback collects for its launches.
struct Fallback {
  std::vector<size_t> entries;     // entries with rc == 0, in batch order
  std::vector<Regions> regions;    // theirs, base relative to the CRC area until placed
  std::vector<GatherRec> gathers;  // src absolute, dst relative to the CRC area
  uint64_t crc_bytes = 0;          // of the CRC area, every entry's first byte 16-byte aligned
};

// The walk of the entry's stream (walk_pieces): every packet's CRC region
// becomes a record of the gather.
int walk_entry(hdfs_md5crc_streams_entry &x, size_t b, int proto, uint32_t chunk_size, int ctype, Fallback &f) {
  x.path = HDFS_MD5CRC_STREAMS_PATH_FALLBACK;
  const uint8_t *s = static_cast<const uint8_t *>(x.stream);
  const size_t first_gather = f.gathers.size();
  const uint64_t area0 = f.crc_bytes;
  uint64_t crc_bytes = 0;
  const Walk w = walk_pieces(g_s.recs, kPieceRecords, s, x.len, b, proto, chunk_size, ctype,
                             [&](const hdfs_crc32c_packet &k, uint64_t at) {
                               if (k.crc_len <= 0) return;
                               f.gathers.push_back(
                                   GatherRec{reinterpret_cast<uintptr_t>(s) + at + k.stream_off + k.header_len,
                                             area0 + crc_bytes, uint32_t(k.crc_len), 0u});
                               crc_bytes += uint64_t(k.crc_len);
                             });
  x.npkts = w.npkts;
  x.payload = w.payload;
  x.offset_in_block = w.offset_in_block;
  x.rc = w.rc;
  if (w.rc >= 0) x.consumed = w.pos;
  if (w.rc) {  // the engine's failure, or a framing error: no digest
    f.gathers.resize(first_gather);
    return w.rc;
  }
  if (crc_bytes / 4u > 0xFFFFFFFFull) {
    f.gathers.resize(first_gather);
    x.rc = HDFS_CRC32C_EINVAL;
    return fail(HDFS_CRC32C_EINVAL, "entry %zu: more than 2^32 - 1 CRCs in one stream", b);
  }
  x.nchunks = crc_bytes / 4u;
  Regions r = Regions{};
  r.base = area0;
  r.limit = crc_bytes;
  r.nwords = x.nchunks;
  r.ntail = 1u;
  r.tail_words0 = uint32_t(x.nchunks);
  r.nblk = uint32_t(hdfs_md5crc::md5_words_blocks(r.nwords));
  r.entry = uint32_t(b);
  f.entries.push_back(b);
  f.regions.push_back(r);
  f.crc_bytes = (area0 + crc_bytes + 15u) & ~uint64_t(15);
  return 0;
}

// The fallback's launches: the records' CRC regions gathered into scratch, then
// the digest kernel over one-region descriptors, the digests back, one
// synchronise.
int digest_fallbacks(hdfs_md5crc_streams_entry *e, Fallback &f, hipStream_t st) {
  const size_t nf = f.entries.size();
  if (!nf) return HDFS_CRC32C_OK;
  if (f.gathers.size() > 0x7FFFFFFFull)
    return fail(HDFS_CRC32C_EINVAL, "entry %zu: too many packets to gather in one call", f.entries[0]);
  // scratch: Regions[nf] | digests[16 nf] | GatherRec[] | the CRC area
  const size_t o_reg = 0, o_dig = o_reg + nf * sizeof(Regions), o_rec = o_dig + nf * 16;
  const size_t o_crc = (o_rec + f.gathers.size() * sizeof(GatherRec) + 15u) & ~size_t(15);
  int rc = g_s.gather.reserve(o_crc + size_t(f.crc_bytes), kScratchFloor);
  if (rc) return rc;
  uint8_t *dv = g_s.gather.as<uint8_t>();
  for (Regions &r : f.regions) r.base += reinterpret_cast<uintptr_t>(dv + o_crc);
  std::vector<uint8_t> dig(nf * 16);
  hipError_t he = hipMemcpyAsync(dv + o_reg, f.regions.data(), nf * sizeof(Regions), hipMemcpyHostToDevice, st);
  if (he == hipSuccess && !f.gathers.empty())
    he = hipMemcpyAsync(dv + o_rec, f.gathers.data(), f.gathers.size() * sizeof(GatherRec), hipMemcpyHostToDevice, st);
  if (he == hipSuccess)
    he = launch_gather_regions(reinterpret_cast<const GatherRec *>(dv + o_rec), uint32_t(f.gathers.size()), dv + o_crc,
                               st);
  if (he == hipSuccess)
    he = launch_digest_streams(reinterpret_cast<const Regions *>(dv + o_reg), nullptr, nullptr, uint32_t(nf),
                               reinterpret_cast<uint32_t *>(dv + o_dig), st);
  if (he == hipSuccess) he = hipMemcpyAsync(dig.data(), dv + o_dig, nf * 16, hipMemcpyDeviceToHost, st);
  rc = sync_and_report(st, he, HDFS_CRC32C_OK, nullptr, "digest of the fallback entries");
  if (rc) return rc;
  for (size_t i = 0; i < nf; i++) std::memcpy(e[f.entries[i]].md5, dig.data() + 16 * i, 16);
  return HDFS_CRC32C_OK;
}

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_md5crc_streams_block_digests.  timing: the
// same on the library's stream, then the three launches alone iters more times
// between two events (hdfs_md5crc_streams_time).
int block_digests(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype, void *stream,
                  bool timing, unsigned flags, int iters, double *ms_per_iter) {
  if (ms_per_iter) *ms_per_iter = 0;
  int rc = check_arguments(e, n, proto, chunk_size, ctype);
  if (rc) return rc;
  if (timing) {  // decided by the arguments alone, before any device is asked
    if ((rc = timing_args_ok(iters, ms_per_iter))) return rc;
    if (flags != HDFS_MD5CRC_STREAMS_TIME_NONE) return fail(HDFS_CRC32C_EINVAL, "unknown timing flags 0x%x", flags);
  }
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_stream_places(e, n, dev))) return rc;
  const Tables T(n);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, T.bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  // the entries, in pinned memory; one without bytes is uploaded empty, so the probe finds it irregular
  uint8_t *pin = g_s.tab.pin.as<uint8_t>(), *dv = g_s.tab.dev.as<uint8_t>();
  Entry *in = reinterpret_cast<Entry *>(pin + T.in);
  uint64_t all = 0;
  for (size_t b = 0; b < n; b++) {
    in[b] = e[b].len ? Entry{static_cast<const uint8_t *>(e[b].stream), e[b].len} : Entry{nullptr, 0};
    all += e[b].len >> 12;
  }
  // a wave of the header check for every 4 KiB of stream, up to the grid's limit
  const uint64_t want = all / kCheckWaves + 1u;
  const uint32_t groups = want < kCheckMaxGroups ? uint32_t(want) : kCheckMaxGroups;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  auto launches = [&] {
    hipError_t le = launch_probe_streams(dv, uint32_t(n), proto, chunk_size, ctype, st);
    if (le == hipSuccess) le = launch_check_headers(dv, uint32_t(n), uint32_t(proto), groups, st);
    if (le == hipSuccess)
      le = launch_digest_streams(reinterpret_cast<const Regions *>(dv + T.reg),
                                 reinterpret_cast<const uint32_t *>(dv + T.status),
                                 reinterpret_cast<const uint32_t *>(dv + T.meta), uint32_t(n),
                                 reinterpret_cast<uint32_t *>(dv + T.digest), st);
    return le;
  };
  if ((rc = probed_run(st, g_s.tab, T.in, n * sizeof(Entry), T.digest, T.bytes, g_s.ev, timing ? iters : 0,
                       ms_per_iter, "md5crc streams", launches)))
    return rc;
  const Desc *desc = reinterpret_cast<const Desc *>(pin + T.desc);
  const Regions *reg = reinterpret_cast<const Regions *>(pin + T.reg);
  const uint8_t *digest = pin + T.digest;
  const uint32_t *slot = reinterpret_cast<const uint32_t *>(pin + T.slot);
  const uint32_t *status = reinterpret_cast<const uint32_t *>(pin + T.status);
  const uint32_t nreg = reinterpret_cast<const uint32_t *>(pin + T.meta)[0];
  Outcomes out;
  Fallback f;
  for (size_t b = 0; b < n; b++) {
    hdfs_md5crc_streams_entry &x = e[b];
    const uint32_t s = slot[b];
    if (!slot_adds_up(s, kNoSlot, nreg, b, [&](uint32_t i) { return desc[i].entry; }) ||
        (s != kNoSlot && reg[s].entry != b))
      return tables_fail(b);
    if (s != kNoSlot && !status[s]) {
      const Desc &d = desc[s];
      x.rc = 0;
      x.path = HDFS_MD5CRC_STREAMS_PATH_KERNEL;
      x.npkts = d.npk;
      x.consumed = d.consumed;
      x.payload = d.delivered;
      x.nchunks = reg[s].nwords;
      x.offset_in_block = d.off0;
      std::memcpy(x.md5, digest + 16 * size_t(s), 16);  // the state's words, little-endian: the digest's bytes
      continue;
    }
    out.note(walk_entry(x, b, proto, chunk_size, ctype, f));
  }
  if ((rc = digest_fallbacks(e, f, st))) return rc;
  return out.result();
}

}  // namespace
}  // namespace hdfs_md5crc_streams

using namespace hdfs_md5crc_streams;

extern "C" {

int hdfs_md5crc_streams_abi_version(void) { return HDFS_MD5CRC_STREAMS_ABI_VERSION; }

const char *hdfs_md5crc_streams_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_md5crc_streams_block_digests(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size,
                                      int ctype, void *stream) {
  return block_digests(e, n, proto, chunk_size, ctype, stream, false, 0u, 0, nullptr);
}

int hdfs_md5crc_streams_file_checksum(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size,
                                      int ctype, void *stream, hdfs_md5crc_file_checksum *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  const int rc = block_digests(e, n, proto, chunk_size, ctype, stream, false, 0u, 0, nullptr);
  if (rc < 0) return rc;
  if (!out) return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry 0: null out");
  if (chunk_size > 0x7FFFFFFFu)
    return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry 0: chunk_size does not fit the s32 wire field");
  for (size_t b = 0; b < n; b++) {
    if (e[b].rc)
      return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry %zu: its stream ends in packet error %d", b, e[b].rc);
    if (e[b].offset_in_block)
      return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry %zu: its stream starts at block offset %lld, not 0", b,
                                  static_cast<long long>(e[b].offset_in_block));
  }
  std::vector<uint32_t> words(4 * n);
  for (size_t b = 0; b < n; b++) std::memcpy(&words[4 * b], e[b].md5, 16);
  out->bytes_per_crc = chunk_size;
  out->ctype = uint32_t(ctype);
  out->crc_per_block = n > 1 ? e[0].nchunks : 0;
  md5_of_words(words.data(), 4 * uint64_t(n), out->md5);
  return HDFS_CRC32C_OK;
}

int hdfs_md5crc_streams_time(hdfs_md5crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                             unsigned flags, int iters, double *ms_per_iter) {
  return block_digests(e, n, proto, chunk_size, ctype, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
