// libhadoofus_crc_streams.so: entry points of include/hadoofus_crc_streams.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Its kernels (crc_streams_kernels.hip) frame the regular entries of a batch,
// check their headers and fold their CRC regions where they lie.  Every other
// entry is framed by hdfs_crc32c_parse_packets, called here after the
// synchronise: this file holds no walk of its own.  The records of that walk
// become a per-packet table that the same kernels fold and reduce.  The host
// combines only whole blocks (hdfs_crc_streams_combine), with
// crc32c_tables.h's operator.  The run, the walk in pieces and the collection
// of the entries' outcomes are read_batch_host.h's.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "companion_support.h"
#include "crc32c_tables.h"
#include "crc_streams_internal.h"
#include "crc_streams_lookup.h"
#include "hadoofus_crc_streams.h"
#include "read_batch_host.h"
#include "read_batch_layout.h"

namespace hdfs_crc_streams {
namespace {

using namespace hdfs_companion;

static_assert(HDFS_CRC_STREAMS_MAX_ENTRIES == kMaxEntries, "the header's limit is the probe's");
static_assert(sizeof(hdfs_crc_streams_entry) == 72, "the ABI of version 1");
static_assert(sizeof(struct hdfs_crc_streams_file_checksum) == 24, "the ABI of version 1");

uint32_t poly_of(int ctype) { return ctype == HDFS_CRC32C_CSUM_CRC32 ? hdfs_crc32c::kPolyZlib : hdfs_crc32c::kPoly; }

// ---- device state -------------------------------------------------------------
// On the engine's device: the call's device tables and their pinned twin, the
// per-packet table and the fallback's scratch (records, spans, CRCs), all grown
// on demand, never shrunk, kept between calls; on the host the multiplier table
// of the checksum type and chunk size used last.  Calls hold g_mu from the
// tables' upload to the last fallback entry, so one call's tables are never
// overwritten under its kernels or under the host's reading of them.
std::mutex g_mu;
struct Scratch : DeviceScratch {
  TablePair tab;
  DeviceBuffer cp;      // a CRC per packet
  DeviceBuffer described;
  std::vector<hdfs_crc32c_packet> recs;  // a fallback entry's records, a piece of the walk at a time
  uint32_t mult[kMultWords];
  int mult_ctype = -1;
  uint32_t mult_chunk = 0;

  int reserve(int to, size_t tab_bytes) {
    const int rc = bind(to, "stream", [this] {
      tab.release();
      cp.release();
      described.release();
    });
    return rc ? rc : tab.reserve(tab_bytes, kTableFloor);
  }

  // The multipliers of (ctype, chunk_size).
  const uint32_t *multipliers(int ctype, uint32_t chunk_size) {
    if (mult_ctype == ctype && mult_chunk == chunk_size) return mult;
    make_multipliers(mult, poly_of(ctype), chunk_size);
    mult_ctype = ctype;
    mult_chunk = chunk_size;
    return mult;
  }
} g_s;

void clear_outputs(hdfs_crc_streams_entry *e, size_t n) {
  for (size_t b = 0; b < n; b++) {
    e[b].consumed = e[b].payload = e[b].nchunks = e[b].npkts = 0;
    e[b].offset_in_block = 0;
    e[b].rc = 0;
    e[b].path = HDFS_CRC_STREAMS_PATH_KERNEL;
    e[b].crc = e[b].reserved = 0;
  }
}

bool ctype_ok(int ctype) { return ctype == HDFS_CRC32C_CSUM_CRC32 || ctype == HDFS_CRC32C_CSUM_CRC32C; }

// ---- argument checks that need no device ------------------------------------------
int check_arguments(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype) {
  if (!e || !n) return fail(HDFS_CRC32C_EINVAL, "entry 0: no entries");
  if (n > kMaxEntries)
    return fail(HDFS_CRC32C_EINVAL, "entry %u: %zu entries, at most %u in one call", unsigned(kMaxEntries), n,
                unsigned(kMaxEntries));
  clear_outputs(e, n);
  if (!packet_args_ok(proto, ctype, 0)) return prefix_fail(HDFS_CRC32C_EINVAL, "entry 0");
  if (!ctype_ok(ctype)) return fail(HDFS_CRC32C_EINVAL, "entry 0: no CRCs to combine without CRC32 or CRC32C");
  if (!chunk_size) return fail(HDFS_CRC32C_EINVAL, "entry 0: chunk_size 0");
  for (size_t b = 0; b < n; b++)
    if (e[b].len && !e[b].stream) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null stream", b);
  return HDFS_CRC32C_OK;
}

// ---- an entry handed to the main library ------------------------------------------------
// What the fallback collects for its launches.
struct Fallback {
  std::vector<size_t> entries;  // entries with rc == 0 and a CRC to fold, in batch order
  std::vector<Span> spans;      // theirs
  std::vector<PktRec> pkts;
};

// The walk of the entry's stream (walk_pieces): every packet with CRCs becomes
// a record of the per-packet table.
int walk_entry(hdfs_crc_streams_entry &x, size_t b, int proto, uint32_t chunk_size, int ctype, Fallback &f) {
  x.path = HDFS_CRC_STREAMS_PATH_FALLBACK;
  const uint8_t *s = static_cast<const uint8_t *>(x.stream);
  const size_t first_pkt = f.pkts.size();
  uint64_t nchunks = 0;
  const Walk w = walk_pieces(g_s.recs, kPieceRecords, s, x.len, b, proto, chunk_size, ctype,
                             [&](const hdfs_crc32c_packet &k, uint64_t at) {
                               if (k.crc_len <= 0) return;
                               f.pkts.push_back(PktRec{reinterpret_cast<uintptr_t>(s) + at + k.stream_off + k.header_len,
                                                       0u, uint32_t(k.crc_len) / 4u, uint32_t(k.data_len)});
                               nchunks += uint32_t(k.crc_len) / 4u;
                             });
  x.npkts = w.npkts;
  x.payload = w.payload;
  x.offset_in_block = w.offset_in_block;
  x.rc = w.rc;
  if (w.rc >= 0) x.consumed = w.pos;
  if (w.rc) {  // the engine's failure, or a framing error: no CRC
    f.pkts.resize(first_pkt);
    return w.rc;
  }
  const size_t npk = f.pkts.size() - first_pkt;
  if (f.pkts.size() > hdfs_read_batch::kMaxPackets) {
    f.pkts.resize(first_pkt);
    x.rc = HDFS_CRC32C_EINVAL;
    return fail(HDFS_CRC32C_EINVAL, "entry %zu: too many packets to fold in one call", b);
  }
  x.nchunks = nchunks;
  if (!npk) return 0;  // no CRC: crc 0
  uint64_t after = 0;
  for (size_t i = f.pkts.size(); i-- > first_pkt;) {
    f.pkts[i].after = after;
    after += f.pkts[i].dlen;
  }
  f.entries.push_back(b);
  f.spans.push_back(Span{uint32_t(first_pkt), uint32_t(npk)});
  return 0;
}

// The fallback's launches: the records' table up, the fold and the reduce over
// described packets, the CRCs back, one synchronise.  mult: the call's
// multiplier table in device memory.
int fold_fallbacks(hdfs_crc_streams_entry *e, Fallback &f, const uint32_t *mult, hipStream_t st) {
  const size_t nf = f.entries.size(), np = f.pkts.size();
  if (!nf) return HDFS_CRC32C_OK;
  // scratch: PktRec[np] | Span[nf] | crc[nf]
  const size_t o_rec = 0, o_span = o_rec + np * sizeof(PktRec), o_crc = o_span + nf * sizeof(Span);
  int rc = g_s.described.reserve(o_crc + nf * sizeof(uint32_t), kScratchFloor);
  if (!rc) rc = g_s.cp.reserve(np * sizeof(uint32_t), kScratchFloor);
  if (rc) return rc;
  uint8_t *dv = g_s.described.as<uint8_t>();
  std::vector<uint32_t> crc(nf);
  const uint64_t want = np / kFoldWaves + 1u;
  const uint32_t groups = want < kFoldMaxGroups ? uint32_t(want) : kFoldMaxGroups;
  hipError_t he = hipMemcpyAsync(dv + o_rec, f.pkts.data(), np * sizeof(PktRec), hipMemcpyHostToDevice, st);
  if (he == hipSuccess)
    he = hipMemcpyAsync(dv + o_span, f.spans.data(), nf * sizeof(Span), hipMemcpyHostToDevice, st);
  if (he == hipSuccess)
    he = launch_fold_described(reinterpret_cast<const PktRec *>(dv + o_rec), uint32_t(np), mult, groups,
                               g_s.cp.as<uint32_t>(), st);
  if (he == hipSuccess)
    he = launch_reduce_described(reinterpret_cast<const Span *>(dv + o_span), uint32_t(nf),
                                 reinterpret_cast<const PktRec *>(dv + o_rec), uint32_t(np), mult,
                                 g_s.cp.as<uint32_t>(), reinterpret_cast<uint32_t *>(dv + o_crc), st);
  if (he == hipSuccess) he = hipMemcpyAsync(crc.data(), dv + o_crc, nf * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  rc = sync_and_report(st, he, HDFS_CRC32C_OK, nullptr, "fold of the fallback entries");
  if (rc) return rc;
  for (size_t i = 0; i < nf; i++) e[f.entries[i]].crc = crc[i];
  return HDFS_CRC32C_OK;
}

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_crc_streams_block_crcs.  timing: the same
// on the library's stream, then the three launches alone iters more times
// between two events (hdfs_crc_streams_time).
int block_crcs(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype, void *stream,
               bool timing, unsigned flags, int iters, double *ms_per_iter) {
  if (ms_per_iter) *ms_per_iter = 0;
  int rc = check_arguments(e, n, proto, chunk_size, ctype);
  if (rc) return rc;
  if (timing) {  // decided by the arguments alone, before any device is asked
    if ((rc = timing_args_ok(iters, ms_per_iter))) return rc;
    if (flags != HDFS_CRC_STREAMS_TIME_NONE) return fail(HDFS_CRC32C_EINVAL, "unknown timing flags 0x%x", flags);
  }
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_stream_places(e, n, dev))) return rc;
  const Tables T(n);
  // the per-packet table, sized from the lengths alone: the probe has not run
  uint64_t all = 0, bound = 0;
  for (size_t b = 0; b < n; b++) {
    all += e[b].len >> 12;
    bound += e[b].len / kMinPacketWire + hdfs_read_batch::kMaxTail;
  }
  const uint32_t cap = bound < kPacketBudget ? uint32_t(bound) : kPacketBudget;
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, T.bytes)) || (rc = g_s.cp.reserve(size_t(cap) * sizeof(uint32_t), kScratchFloor)) ||
      (timing && (rc = g_s.timing_events())))
    return rc;
  // the entries and the multipliers, in pinned memory; an entry without bytes is uploaded empty, so the probe
  // finds it irregular
  uint8_t *pin = g_s.tab.pin.as<uint8_t>(), *dv = g_s.tab.dev.as<uint8_t>();
  Entry *in = reinterpret_cast<Entry *>(pin + T.in);
  for (size_t b = 0; b < n; b++)
    in[b] = e[b].len ? Entry{static_cast<const uint8_t *>(e[b].stream), e[b].len} : Entry{nullptr, 0};
  std::memcpy(pin + T.mult, g_s.multipliers(ctype, chunk_size), kMultWords * sizeof(uint32_t));
  // a wave of the fold for every 4 KiB of stream, up to the grid's limit
  const uint64_t want = all / kFoldWaves + 1u;
  const uint32_t groups = want < kFoldMaxGroups ? uint32_t(want) : kFoldMaxGroups;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  uint32_t *cp = g_s.cp.as<uint32_t>();
  auto launches = [&] {
    hipError_t le = launch_probe_streams(dv, uint32_t(n), proto, chunk_size, ctype, st);
    if (le == hipSuccess) le = launch_fold_streams(dv, uint32_t(n), uint32_t(proto), groups, cp, cap, st);
    if (le == hipSuccess) le = launch_reduce_streams(dv, uint32_t(n), cp, cap, st);
    return le;
  };
  if ((rc = probed_run(st, g_s.tab, T.in, T.desc - T.in, T.desc, T.bytes, g_s.ev, timing ? iters : 0, ms_per_iter,
                       "crc streams", launches)))
    return rc;
  const Desc *desc = reinterpret_cast<const Desc *>(pin + T.desc);
  const uint32_t *crc = reinterpret_cast<const uint32_t *>(pin + T.crc);
  const uint32_t *slot = reinterpret_cast<const uint32_t *>(pin + T.slot);
  const uint32_t *status = reinterpret_cast<const uint32_t *>(pin + T.status);
  const uint32_t *pk0 = reinterpret_cast<const uint32_t *>(pin + T.pk0);
  const uint32_t nreg = reinterpret_cast<const uint32_t *>(pin + T.meta)[0];
  Outcomes out;
  Fallback f;
  for (size_t b = 0; b < n; b++) {
    hdfs_crc_streams_entry &x = e[b];
    const uint32_t s = slot[b];
    if (!slot_adds_up(s, kNoSlot, nreg, b, [&](uint32_t i) { return desc[i].entry; })) return tables_fail(b);
    if (s != kNoSlot && !status[s] && pk0[s + 1] <= cap) {
      const Desc &d = desc[s];
      x.rc = 0;
      x.path = HDFS_CRC_STREAMS_PATH_KERNEL;
      x.npkts = d.npk;
      x.consumed = d.consumed;
      x.payload = d.delivered;
      x.nchunks = uint64_t(d.nbody) * hdfs_read_batch::crc_count(d.dlen0);
      for (uint32_t t = 0; t < d.ntail; t++) x.nchunks += hdfs_read_batch::crc_count(d.tail[t].dlen);
      x.offset_in_block = d.off0;
      x.crc = crc[s];
      continue;
    }
    out.note(walk_entry(x, b, proto, chunk_size, ctype, f));
  }
  if ((rc = fold_fallbacks(e, f, reinterpret_cast<const uint32_t *>(dv + T.mult), st))) return rc;
  return out.result();
}

int combine(const uint32_t *crcs, const uint64_t *lens, size_t n, int ctype, uint32_t *out) {
  if (out) *out = 0;
  if (!out || (n && (!crcs || !lens))) return fail(HDFS_CRC32C_EINVAL, "combine: null pointer");
  if (!ctype_ok(ctype)) return fail(HDFS_CRC32C_EINVAL, "combine: bad checksum type %d", ctype);
  const uint32_t poly = poly_of(ctype);
  uint32_t acc = 0;
  for (size_t i = 0; i < n; i++) acc = hdfs_crc32c::zeros_op(lens[i], poly).apply(acc) ^ crcs[i];
  *out = acc;
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_crc_streams

using namespace hdfs_crc_streams;

extern "C" {

int hdfs_crc_streams_abi_version(void) { return HDFS_CRC_STREAMS_ABI_VERSION; }

const char *hdfs_crc_streams_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_crc_streams_block_crcs(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                                void *stream) {
  return block_crcs(e, n, proto, chunk_size, ctype, stream, false, 0u, 0, nullptr);
}

int hdfs_crc_streams_combine(const uint32_t *crcs, const uint64_t *lens, size_t n, int ctype, uint32_t *out) {
  return combine(crcs, lens, n, ctype, out);
}

int hdfs_crc_streams_file_checksum(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                                   void *stream, struct hdfs_crc_streams_file_checksum *out) {
  if (out) std::memset(out, 0, sizeof(*out));
  const int rc = block_crcs(e, n, proto, chunk_size, ctype, stream, false, 0u, 0, nullptr);
  if (rc < 0) return rc;
  if (!out) return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry 0: null out");
  for (size_t b = 0; b < n; b++) {
    if (e[b].rc)
      return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry %zu: its stream ends in packet error %d", b, e[b].rc);
    if (e[b].offset_in_block)
      return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "entry %zu: its stream starts at block offset %lld, not 0", b,
                                  static_cast<long long>(e[b].offset_in_block));
  }
  std::vector<uint32_t> crcs(n);
  std::vector<uint64_t> lens(n);
  uint64_t length = 0;
  for (size_t b = 0; b < n; b++) {
    crcs[b] = e[b].crc;
    lens[b] = e[b].payload;
    length += e[b].payload;
  }
  uint32_t crc = 0;
  const int cr = combine(crcs.data(), lens.data(), n, ctype, &crc);
  if (cr) return cr;
  out->bytes_per_crc = chunk_size;
  out->ctype = uint32_t(ctype);
  out->crc = crc;
  for (int k = 0; k < 4; k++) out->bytes[k] = uint8_t(crc >> (24 - 8 * k));
  out->length = length;
  return HDFS_CRC32C_OK;
}

int hdfs_crc_streams_time(hdfs_crc_streams_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                          unsigned flags, int iters, double *ms_per_iter) {
  return block_crcs(e, n, proto, chunk_size, ctype, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
