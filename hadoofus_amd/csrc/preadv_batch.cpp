// libhadoofus_preadv_batch.so: entry points of include/hadoofus_preadv_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Its kernels (preadv_batch_kernels.hip) frame and verify the packets the
// regular entries' reads take and lay the bytes of their windows over the
// entries' device fragments; the CRC tables are the fused write libraries'
// (wire_fused_host.h, built out of crc32c_tables.h).  Every other entry is
// hdfs_crc32c_read_packets' work, called here after the synchronise with the
// entry's own fragment list: this file holds no walk of its own.  The records
// of a regular entry follow from its descriptor, cut by the probe to the
// packets the read takes (pread_batch_layout.h; read_batch_layout.h:
// packet_of, record_of).  The run, the collection of the entries' outcomes and
// the scratch are read_batch_host.h's, the overlap sweep companion_support.h's.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "companion_support.h"
#include "hadoofus_preadv_batch.h"
#include "pread_batch_layout.h"
#include "preadv_batch_internal.h"
#include "read_batch_host.h"
#include "wire_fused_host.h"
#include "wire_fused_tables.h"

namespace hdfs_preadv_batch {
namespace {

using namespace hdfs_companion;
using hdfs_pread_batch::packet_of;
using hdfs_pread_batch::record_of;

static_assert(HDFS_PREADV_BATCH_MAX_ENTRIES == kMaxEntries, "the header's limit is the probe's");

// ---- device state -------------------------------------------------------------
// On the engine's device: the CRC tables and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept;
// the call's device tables and their pinned twin, grown on demand, never
// shrunk, kept between calls.  Calls hold g_mu from the tables' upload to the
// last fallback entry, so one call's tables are never overwritten under its
// kernels or under the host's reading of them.
std::mutex g_mu;
using Fused = hdfs_wire_fused::DeviceState<prepare_unframe_scatter_batch, kBatchMaxGroups>;
ReadScratch<Fused> g_s;

void clear_outputs(hdfs_preadv_batch_entry *e, size_t n) {
  for (size_t b = 0; b < n; b++) {
    e[b].consumed = e[b].delivered = e[b].npkts = 0;
    e[b].rc = 0;
    e[b].path = HDFS_PREADV_BATCH_PATH_FALLBACK;
  }
}

// What the fragment lists of a call add up to.
struct Shape {
  std::vector<uint64_t> cap;  // per entry: the total of its fragments
  size_t nfe = 0;             // rows of the fragment table, every entry's sentinel included
};

// An entry without a stream or without room names no range: the main call
// answers it without looking at either.
bool has_ranges(const hdfs_preadv_batch_entry &x, uint64_t cap) { return x.len && cap; }

// ---- argument checks that need no device ------------------------------------------
// Counts and limits first, every entry's; then the fragment arrays (host
// memory) are read, no device pointer is looked at.
int check_arguments(hdfs_preadv_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype, Shape &sh) {
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
    if (e[b].read_len == HDFS_CRC32C_READ_ALL)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: whole payloads (READ_ALL) are hdfs_read_batch_read_blocks' job", b);
    if (e[b].read_len <= 0)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: read_len %lld, a read window has at least one byte", b,
                  (long long)e[b].read_len);
    if (e[b].iovcnt < 1 || !e[b].iov)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: iovcnt %d%s, a read has at least one fragment", b, int(e[b].iovcnt),
                  e[b].iov ? "" : " and a null iov");
  }
  sh.cap.assign(n, 0);
  sh.nfe = n;
  size_t nonempty = 0;
  for (size_t b = 0; b < n; b++) {
    uint64_t cap = 0;
    size_t mine = 0;
    for (int32_t i = 0; i < e[b].iovcnt; i++) {
      const hdfs_crc32c_iovec &f = e[b].iov[i];
      if (!f.len) continue;
      if (!f.base)
        return fail(HDFS_CRC32C_EINVAL, "entry %zu: fragment %d: null base with %llu bytes", b, int(i),
                    (unsigned long long)f.len);
      if (cap + f.len < cap)
        return fail(HDFS_CRC32C_EINVAL, "entry %zu: fragment %d: the fragments' lengths overflow", b, int(i));
      cap += f.len;
      if (++nonempty > HDFS_PREADV_BATCH_MAX_FRAGS)
        return fail(HDFS_CRC32C_EINVAL, "entry %zu: fragment %d: more than %u non-empty fragments in one call", b,
                    int(i), unsigned(HDFS_PREADV_BATCH_MAX_FRAGS));
      mine++;
    }
    sh.cap[b] = cap;
    if (has_ranges(e[b], cap)) sh.nfe += mine;
  }
  return HDFS_CRC32C_OK;
}

// ---- where the buffers lie -----------------------------------------------------------
// Every range inside one allocation of device `dev`; no non-empty fragment
// overlaps a stream or another fragment of the batch, the same entry's
// included.  A call may hold millions of fragments, so the overlaps are found
// by one sweep over the sorted ranges (check_overlaps, one Span per fragment
// and per stream), not by comparing every pair.
int check_batch_places(const hdfs_preadv_batch_entry *e, size_t n, const Shape &sh, int dev) {
  int rc;
  Allocations al;
  std::vector<Span> frags, streams;
  frags.reserve(sh.nfe);
  streams.reserve(n);
  for (size_t b = 0; b < n; b++) {
    if (!has_ranges(e[b], sh.cap[b])) continue;
    if ((rc = al.check(e[b].stream, e[b].len, dev, "stream"))) return prefix_fail(rc, "entry %zu", b);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(e[b].stream);
    streams.push_back(Span{s0, s0 + uintptr_t(e[b].len), uint32_t(b), 0u});
    for (int32_t i = 0; i < e[b].iovcnt; i++) {
      const hdfs_crc32c_iovec &f = e[b].iov[i];
      if (!f.len) continue;
      if ((rc = al.check(f.base, f.len, dev, "base"))) return prefix_fail(rc, "entry %zu: fragment %d", b, int(i));
      const uintptr_t d0 = reinterpret_cast<uintptr_t>(f.base);
      frags.push_back(Span{d0, d0 + uintptr_t(f.len), uint32_t(b), 1u});
    }
  }
  // Fragments given in rising address order (the rows of a tensor, say) need no sort: one pass says so.
  Span sw, so;
  if (!(rc = check_overlaps(frags, streams, &sw, &so))) return rc;
  // say which fragments: a span's is the first of its entry with that range, but for `skip`
  const auto frag_of = [&](const Span &s, int32_t skip) {
    for (int32_t i = 0; i < e[s.k].iovcnt; i++) {
      const hdfs_crc32c_iovec &f = e[s.k].iov[i];
      const uintptr_t a = reinterpret_cast<uintptr_t>(f.base);
      if (f.len && i != skip && a == s.lo && a + uintptr_t(f.len) == s.hi) return i;
    }
    return skip;
  };
  const int32_t fw = frag_of(sw, -1);
  if (!so.wire)
    return fail(rc, "entry %u: fragment %d overlaps the stream of entry %u", sw.k, int(fw), so.k);
  const int32_t fo = frag_of(so, so.k == sw.k ? fw : -1);  // one entry's fragment given twice: the other of the two
  const bool later = sw.k > so.k || (sw.k == so.k && fw > fo);
  return later ? fail(rc, "entry %u: fragment %d overlaps fragment %d of entry %u", sw.k, int(fw), int(fo), so.k)
               : fail(rc, "entry %u: fragment %d overlaps fragment %d of entry %u", so.k, int(fo), int(fw), sw.k);
}

// ---- an entry handed to the main library ------------------------------------------------
// Exactly the call of the contract (read_unlimited: without a record array of
// the caller's the walk is not cut).
int fallback(hdfs_preadv_batch_entry &x, size_t b, int proto, uint32_t chunk_size, int ctype,
             hdfs_crc32c_packet *pkts, size_t max_pkts) {
  size_t np = 0;
  uint64_t used = 0, got = 0;
  const int rc = read_unlimited(g_s.recs, x.stream, x.len, proto, chunk_size, ctype, x.client_offset, x.read_len, x.iov,
                                x.iovcnt, pkts ? pkts + b * max_pkts : nullptr, max_pkts, &np, &used, &got);
  x.rc = rc;
  x.path = HDFS_PREADV_BATCH_PATH_FALLBACK;
  if (rc < 0) return engine_fail(rc, "read_packets"), prefix_fail(rc, "entry %zu", b);
  x.npkts = np;
  x.consumed = used;
  x.delivered = got;
  return rc;
}

// ---- the tables of a call -----------------------------------------------------------------
// The fragment table, fr0 and the entries, in pinned memory.  An entry without
// ranges is uploaded empty, so the probe finds it irregular; its slice is its
// sentinel alone.
void fill_tables(uint8_t *pin, const Tables &T, const hdfs_preadv_batch_entry *e, size_t n, const Shape &sh) {
  Frag *ft = reinterpret_cast<Frag *>(pin + T.ft);
  uint32_t *fr0 = reinterpret_cast<uint32_t *>(pin + T.fr0);
  Entry *in = reinterpret_cast<Entry *>(pin + T.base + T.p.in);
  uint32_t row = 0;
  for (size_t b = 0; b < n; b++) {
    const bool has = has_ranges(e[b], sh.cap[b]);
    fr0[b] = row;
    uint64_t at = 0;
    for (int32_t i = 0; has && i < e[b].iovcnt; i++) {
      const hdfs_crc32c_iovec &f = e[b].iov[i];
      if (!f.len) continue;
      ft[row++] = Frag{static_cast<const uint8_t *>(f.base), at};
      at += f.len;
    }
    ft[row++] = Frag{nullptr, at};
    in[b] = has ? Entry{static_cast<const uint8_t *>(e[b].stream), e[b].len, nullptr, sh.cap[b], e[b].client_offset,
                        e[b].read_len}
                : Entry{nullptr, 0, nullptr, 0, 0, 0};
  }
  fr0[n] = row;  // == sh.nfe
}

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_preadv_batch_read.  timing: the same
// on the library's stream, then both launches alone iters more times between
// two events (hdfs_preadv_batch_time).
int read_windows(hdfs_preadv_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                 hdfs_crc32c_packet *pkts, size_t max_pkts, void *stream, bool timing, unsigned flags, int iters,
                 double *ms_per_iter) {
  if (ms_per_iter) *ms_per_iter = 0;
  Shape sh;
  int rc = check_arguments(e, n, proto, chunk_size, ctype, sh);
  if (rc) return rc;
  if (timing) {  // decided by the arguments alone, before any device is asked
    if ((rc = timing_args_ok(iters, ms_per_iter)) || (rc = Fused::flags_ok(flags))) return rc;
  }
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_batch_places(e, n, sh, dev))) return rc;
  const Tables T(n, sh.nfe);
  const uint32_t nfe = uint32_t(sh.nfe);  // <= 2^22 + 1024
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, T.bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  uint8_t *pin = g_s.tab.pin.as<uint8_t>(), *dv = g_s.tab.dev.as<uint8_t>();
  fill_tables(pin, T, e, n, sh);
  const uint32_t *crc_tab = g_s.fused.tables(ctype);
  const uint32_t groups = (flags >> 8) ? (flags >> 8) : g_s.fused.groups;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  auto launches = [&] {
    hipError_t le = launch_probe(dv, uint32_t(n), nfe, proto, chunk_size, ctype, pkts != nullptr, max_pkts, st);
    if (le == hipSuccess)
      le = launch_unframe_scatter_batch(dv, uint32_t(n), nfe, uint32_t(proto), crc_tab, groups, st);
    return le;
  };
  const size_t back = T.base + T.p.desc;  // what the probe writes starts here
  if ((rc = probed_run(st, g_s.tab, 0, T.up, back, T.bytes, g_s.ev, timing ? iters : 0, ms_per_iter, "preadv batch",
                       launches)))
    return rc;
  const uint8_t *pb = pin + T.base;
  const Window *desc = reinterpret_cast<const Window *>(pb + T.p.desc);
  const uint32_t *slot = reinterpret_cast<const uint32_t *>(pb + T.p.slot);
  const uint32_t *status = reinterpret_cast<const uint32_t *>(pb + T.p.status);
  const uint32_t nreg = reinterpret_cast<const uint32_t *>(pb + T.p.meta)[0];
  Outcomes out;
  for (size_t b = 0; b < n; b++) {
    hdfs_preadv_batch_entry &x = e[b];
    const uint32_t s = slot[b];
    if (!slot_adds_up(s, kNoSlot, nreg, b, [&](uint32_t i) { return desc[i].d.entry; })) return tables_fail(b);
    if (s != kNoSlot && !status[s]) {
      const Desc &d = desc[s].d;
      x.rc = 0;
      x.path = HDFS_PREADV_BATCH_PATH_KERNEL;
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
}  // namespace hdfs_preadv_batch

using namespace hdfs_preadv_batch;

extern "C" {

int hdfs_preadv_batch_abi_version(void) { return HDFS_PREADV_BATCH_ABI_VERSION; }

const char *hdfs_preadv_batch_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_preadv_batch_read(hdfs_preadv_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                           hdfs_crc32c_packet *pkts, size_t max_pkts, void *stream) {
  return read_windows(e, n, proto, chunk_size, ctype, pkts, max_pkts, stream, false, 0u, 0, nullptr);
}

int hdfs_preadv_batch_time(hdfs_preadv_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                           unsigned flags, int iters, double *ms_per_iter) {
  return read_windows(e, n, proto, chunk_size, ctype, nullptr, 0, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
