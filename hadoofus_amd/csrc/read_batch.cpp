// libhadoofus_read_batch.so: entry points of include/hadoofus_read_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Its kernels (read_batch_kernels.hip) frame, verify and de-frame the regular
// entries of a batch; the CRC tables are the fused write libraries'
// (wire_fused_host.h, built out of crc32c_tables.h).  Every other entry is
// hdfs_crc32c_read_packets' work, called here after the synchronise: this
// file holds no walk of its own.  The records of a regular entry follow from
// its descriptor (read_batch_layout.h: packet_of, record_of).  The run, the
// collection of the entries' outcomes and the scratch are read_batch_host.h's,
// the overlap sweep companion_support.h's.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "companion_support.h"
#include "hadoofus_read_batch.h"
#include "read_batch_host.h"
#include "read_batch_internal.h"
#include "read_batch_layout.h"
#include "wire_fused_host.h"
#include "wire_fused_tables.h"

namespace hdfs_read_batch {
namespace {

using namespace hdfs_companion;

static_assert(HDFS_READ_BATCH_MAX_ENTRIES == kMaxEntries, "the header's limit is the probe's");

// ---- device state -------------------------------------------------------------
// On the engine's device: the CRC tables and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept;
// the call's device tables and their pinned twin, grown on demand, never
// shrunk, kept between calls.  Calls hold g_mu from the tables' upload to the
// last fallback entry, so one call's tables are never overwritten under its
// kernels or under the host's reading of them.
std::mutex g_mu;
using Fused = hdfs_wire_fused::DeviceState<prepare_unframe_fused_batch, kBatchMaxGroups>;
ReadScratch<Fused> g_s;

void clear_outputs(hdfs_read_batch_entry *e, size_t n) {
  for (size_t b = 0; b < n; b++) {
    e[b].consumed = e[b].delivered = e[b].npkts = 0;
    e[b].rc = 0;
    e[b].path = HDFS_READ_BATCH_PATH_FALLBACK;
  }
}

// ---- argument checks that need no device ------------------------------------------
int check_arguments(hdfs_read_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype) {
  if (!e || !n) return fail(HDFS_CRC32C_EINVAL, "no entries");
  if (n > kMaxEntries)
    return fail(HDFS_CRC32C_EINVAL, "%zu entries, at most %u in one call", n, unsigned(kMaxEntries));
  clear_outputs(e, n);
  if (!packet_args_ok(proto, ctype, 0)) return prefix_fail(HDFS_CRC32C_EINVAL, "entry 0");
  if (ctype == HDFS_CRC32C_CSUM_NULL)
    return fail(HDFS_CRC32C_EINVAL, "entry 0: verify + copy-out needs CRC32 or CRC32C");
  if (!chunk_size) return fail(HDFS_CRC32C_EINVAL, "entry 0: chunk_size 0");
  for (size_t b = 0; b < n; b++) {
    if (e[b].len && !e[b].stream) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null stream", b);
    if (e[b].len && e[b].dst_cap && !e[b].dst) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null destination", b);
  }
  return HDFS_CRC32C_OK;
}

// An entry without a stream or without room names no range: the main call
// answers it without looking at either.
bool has_ranges(const hdfs_read_batch_entry &x) { return x.len && x.dst_cap; }

// ---- where the buffers lie -----------------------------------------------------------
// Every range inside one allocation of device `dev`; no destination overlaps a
// stream or another destination.
int check_batch_places(const hdfs_read_batch_entry *e, size_t n, int dev) {
  int rc;
  Allocations al;
  std::vector<Span> dsts, streams;
  dsts.reserve(n);
  streams.reserve(n);
  for (size_t b = 0; b < n; b++) {
    if (!has_ranges(e[b])) continue;
    if ((rc = al.check(e[b].stream, e[b].len, dev, "stream")) || (rc = al.check(e[b].dst, e[b].dst_cap, dev, "dst")))
      return prefix_fail(rc, "entry %zu", b);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(e[b].stream), d0 = reinterpret_cast<uintptr_t>(e[b].dst);
    streams.push_back(Span{s0, s0 + uintptr_t(e[b].len), uint32_t(b), 0u});
    dsts.push_back(Span{d0, d0 + uintptr_t(e[b].dst_cap), uint32_t(b), 1u});
  }
  return check_overlaps(dsts, streams, nullptr, nullptr, SpanNouns{"dst", "stream"});
}

// ---- an entry handed to the main library ------------------------------------------------
// Exactly the call of the contract (read_unlimited: without a record array of
// the caller's the walk is not cut).
int fallback(hdfs_read_batch_entry &x, size_t b, int proto, uint32_t chunk_size, int ctype, hdfs_crc32c_packet *pkts,
             size_t max_pkts) {
  const hdfs_crc32c_iovec iov{x.dst, x.dst_cap};
  size_t np = 0;
  uint64_t used = 0, got = 0;
  const int rc = read_unlimited(g_s.recs, x.stream, x.len, proto, chunk_size, ctype, 0, HDFS_CRC32C_READ_ALL, &iov, 1,
                                pkts ? pkts + b * max_pkts : nullptr, max_pkts, &np, &used, &got);
  x.rc = rc;
  x.path = HDFS_READ_BATCH_PATH_FALLBACK;
  if (rc < 0) return engine_fail(rc, "read_packets"), prefix_fail(rc, "entry %zu", b);
  x.npkts = np;
  x.consumed = used;
  x.delivered = got;
  return rc;
}

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_read_batch_read_blocks.  timing: the same
// on the library's stream, then both launches alone iters more times between
// two events (hdfs_read_batch_time).
int read_blocks(hdfs_read_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype, hdfs_crc32c_packet *pkts,
                size_t max_pkts, void *stream, bool timing, unsigned flags, int iters, double *ms_per_iter) {
  if (ms_per_iter) *ms_per_iter = 0;
  int rc = check_arguments(e, n, proto, chunk_size, ctype);
  if (rc) return rc;
  if (timing) {  // decided by the arguments alone, before any device is asked
    if ((rc = timing_args_ok(iters, ms_per_iter)) || (rc = Fused::flags_ok(flags))) return rc;
  }
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_batch_places(e, n, dev))) return rc;
  const Tables T(n);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, T.bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  // the entries, in pinned memory; one without ranges is uploaded empty, so the probe finds it irregular
  uint8_t *pin = g_s.tab.pin.as<uint8_t>(), *dv = g_s.tab.dev.as<uint8_t>();
  Entry *in = reinterpret_cast<Entry *>(pin + T.in);
  for (size_t b = 0; b < n; b++)
    in[b] = has_ranges(e[b]) ? Entry{static_cast<const uint8_t *>(e[b].stream), e[b].len,
                                     static_cast<uint8_t *>(e[b].dst), e[b].dst_cap}
                             : Entry{nullptr, 0, nullptr, 0};
  const uint32_t *crc_tab = g_s.fused.tables(ctype);
  const uint32_t groups = (flags >> 8) ? (flags >> 8) : g_s.fused.groups;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  auto launches = [&] {
    hipError_t le = launch_probe(dv, uint32_t(n), proto, chunk_size, ctype, pkts != nullptr, max_pkts, st);
    if (le == hipSuccess) le = launch_unframe_fused_batch(dv, uint32_t(n), uint32_t(proto), crc_tab, groups, st);
    return le;
  };
  if ((rc = probed_run(st, g_s.tab, T.in, n * sizeof(Entry), T.desc, T.bytes, g_s.ev, timing ? iters : 0, ms_per_iter,
                       "read batch", launches)))
    return rc;
  const Desc *desc = reinterpret_cast<const Desc *>(pin + T.desc);
  const uint32_t *slot = reinterpret_cast<const uint32_t *>(pin + T.slot);
  const uint32_t *status = reinterpret_cast<const uint32_t *>(pin + T.status);
  const uint32_t nreg = reinterpret_cast<const uint32_t *>(pin + T.meta)[0];
  Outcomes out;
  for (size_t b = 0; b < n; b++) {
    hdfs_read_batch_entry &x = e[b];
    const uint32_t s = slot[b];
    if (!slot_adds_up(s, kNoSlot, nreg, b, [&](uint32_t i) { return desc[i].entry; })) return tables_fail(b);
    if (s != kNoSlot && !status[s]) {
      const Desc &d = desc[s];
      x.rc = 0;
      x.path = HDFS_READ_BATCH_PATH_KERNEL;
      x.npkts = d.npk;
      x.consumed = d.consumed;
      x.delivered = d.delivered;
      if (pkts)
        for (uint32_t i = 0; i < d.npk; i++) pkts[b * max_pkts + i] = record_of(packet_of(d, i));
      continue;
    }
    out.note(fallback(x, b, proto, chunk_size, ctype, pkts, max_pkts));
  }
  return out.result();
}

}  // namespace
}  // namespace hdfs_read_batch

using namespace hdfs_read_batch;

extern "C" {

int hdfs_read_batch_abi_version(void) { return HDFS_READ_BATCH_ABI_VERSION; }

const char *hdfs_read_batch_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_read_batch_read_blocks(hdfs_read_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                                hdfs_crc32c_packet *pkts, size_t max_pkts, void *stream) {
  return read_blocks(e, n, proto, chunk_size, ctype, pkts, max_pkts, stream, false, 0u, 0, nullptr);
}

int hdfs_read_batch_time(hdfs_read_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype, unsigned flags,
                         int iters, double *ms_per_iter) {
  return read_blocks(e, n, proto, chunk_size, ctype, nullptr, 0, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
