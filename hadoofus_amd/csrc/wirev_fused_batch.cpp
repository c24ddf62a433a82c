// libhadoofus_wirev_fused_batch.so: entry points of
// include/hadoofus_wirev_fused_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// It asks that library for no CRC and has no gather layout: its kernel
// (frame_fused_gather_batch_kernel) computes the chunk CRCs of every write of
// the batch from the bytes it copies out of the fragments, from tables
// (wire_fused_host.h) built out of crc32c_tables.h, and finds the writes and
// their fragments through tables uploaded once per call.  The layout of a
// write and its records are wire_layout.h's; a batch's front end is
// wire_batch_layout.h's, run on a private entry per write whose len is the
// sum of the write's fragments; the rounds are counted by
// wirev_fused_lookup.h's count_packet.  It links no other companion.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "crc32c_outpkt.h"
#include "hadoofus_wirev_fused_batch.h"
#include "wire_batch_layout.h"
#include "wire_fused_host.h"
#include "wire_fused_tables.h"
#include "wire_layout.h"
#include "wirev_fused_batch_internal.h"
#include "wirev_fused_lookup.h"

namespace hdfs_wirev_fused_batch {
namespace {

using namespace hdfs_wire;  // the layout of a write, its records, the batch front end, the timed run
using hdfs_wirev_fused::count_packet;
using hdfs_wirev_fused::RoundCounts;

constexpr uint64_t kMaxPackets = 0x7FFFFFFFull / 4u;  // (2^31 - 1) / 4, the other batch libraries' limit

// The entry wire_batch_layout.h lays out: hdfs_wire_batch_write's fields.
// data stands for the fragment list (the host array, never dereferenced
// there): not NULL wherever the write has bytes.
struct Entry {
  const void *data;
  uint64_t len;
  int64_t offset_in_block;
  int64_t seqno;
  int32_t finish;
  int32_t reserved;
  void *wire;
  uint64_t wire_cap;
  uint64_t wire_len;
  uint64_t npkts;
  uint64_t first_pkt;
};

// ---- layout of the batch ------------------------------------------------------------
// Where every non-empty fragment of every entry starts in its write: entry
// k's slice is at[first[k] .. first[k + 1]), its non-empty fragments' offsets,
// rising strictly from 0, and the write's length behind them (the `at` column
// of the kernel's table, the entries without packets included here).
struct Gather {
  std::vector<Entry> E;
  std::vector<uint64_t> at;
  std::vector<size_t> first;  // n + 1
  uint64_t nfrags = 0;        // non-empty fragments of all entries
  uint32_t nf(size_t k) const { return uint32_t(first[k + 1] - first[k] - 1); }
};

int fragment_fail(int rc, size_t k, int i) {
  prefix_fail(rc, "fragment %d", i);
  return entry_fail(rc, k);
}

// Sums every entry's fragments (only their lengths are read), then lays the
// batch out through the shared front end.  Fills the out fields of every
// entry and the totals.  The limits are judged first, in closed form.
int layout_batch(hdfs_wirev_fused_batch_write *w, size_t n, int proto, int ctype, Batch &B, Gather &G) {
  if (n <= size_t(HDFS_WIREV_FUSED_BATCH_MAX_WRITES) && w) {
    G.E.resize(n);
    G.first.reserve(n + 1);
    for (size_t k = 0; k < n; k++) w[k].len = w[k].wire_len = w[k].npkts = w[k].first_pkt = 0;
    for (size_t k = 0; k < n; k++) {
      const hdfs_crc32c_iovec *iov = w[k].iov;
      if (w[k].iovcnt < 0) return fail(HDFS_CRC32C_EINVAL, "entry %zu: negative fragment count %d", k, w[k].iovcnt);
      if (w[k].iovcnt && !iov) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null fragment list", k);
      G.first.push_back(G.at.size());
      uint64_t total = 0;
      for (int i = 0; i < w[k].iovcnt; i++) {
        const uint64_t l = iov[i].len;
        if (l > (uint64_t(1) << 62) - total) {
          fail(HDFS_CRC32C_EINVAL, "the write's length overflows");
          return fragment_fail(HDFS_CRC32C_EINVAL, k, i);
        }
        if (l) G.at.push_back(total);
        total += l;
      }
      G.nfrags = G.at.size() - k;  // k sentinels so far
      if (G.nfrags > HDFS_WIREV_FUSED_BATCH_MAX_FRAGS)
        return fail(HDFS_CRC32C_EINVAL, "entry %zu: more than %u fragments in the batch", k,
                    HDFS_WIREV_FUSED_BATCH_MAX_FRAGS);
      G.at.push_back(total);
      w[k].len = total;
      G.E[k] = Entry{total ? iov : nullptr, total, w[k].offset_in_block, w[k].seqno, w[k].finish, 0, w[k].wire,
                     w[k].wire_cap, 0, 0, 0};
    }
    G.first.push_back(G.at.size());
  }
  // (with too many writes or none given, the front end says so)
  Counts c;
  int rc = count_batch(w ? G.E.data() : nullptr, n, HDFS_WIREV_FUSED_BATCH_MAX_WRITES, proto, ctype, c);
  if (rc) return rc;
  if (c.packets > kMaxPackets)
    return fail(HDFS_CRC32C_EINVAL, "%llu packets in the batch, at most %llu", (unsigned long long)c.packets,
                (unsigned long long)kMaxPackets);
  rc = layout_entries(G.E.data(), n, proto, ctype, B);
  for (size_t k = 0; k < n; k++) {
    w[k].wire_len = G.E[k].wire_len;
    w[k].npkts = G.E[k].npkts;
    w[k].first_pkt = G.E[k].first_pkt;
  }
  if (rc) return rc;
  if (B.npkts != c.packets) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's packet counts do not add up");
  return HDFS_CRC32C_OK;
}

// ---- where the buffers live -------------------------------------------------------
// Every non-empty fragment and every stream inside one allocation of device
// `dev` each, and no stream over another stream or over any fragment of any
// entry (check_overlaps, one Span per fragment and per stream).
int check_gather_places(const hdfs_wirev_fused_batch_write *w, size_t n, uint64_t nfrags, int dev) {
  int rc;
  Allocations al;
  std::vector<Span> data, wires, spans;
  data.reserve(size_t(nfrags));
  wires.reserve(n);
  for (size_t k = 0; k < n; k++) {
    for (int i = 0; i < w[k].iovcnt; i++) {
      const hdfs_crc32c_iovec &f = w[k].iov[i];
      if (!f.len) continue;
      if ((rc = al.check(f.base, f.len, dev, "data"))) return fragment_fail(rc, k, i);
      const uintptr_t a = reinterpret_cast<uintptr_t>(f.base);
      data.push_back(Span{a, a + uintptr_t(f.len), uint32_t(k), 0u});
    }
    if (w[k].wire_len) {
      if ((rc = al.check(w[k].wire, w[k].wire_len, dev, "wire"))) return entry_fail(rc, k);
      const uintptr_t b = reinterpret_cast<uintptr_t>(w[k].wire);
      wires.push_back(Span{b, b + uintptr_t(w[k].wire_len), uint32_t(k), 1u});
    }
  }
  // Handed over in the sweep's order, which costs a pass where the fragments and the streams each rise in address as
  // they come (a sort of every span, millions of them at most, where they do not).
  for (std::vector<Span> *v : {&data, &wires})
    if (!std::is_sorted(v->begin(), v->end(), span_before)) std::sort(v->begin(), v->end(), span_before);
  spans.resize(data.size() + wires.size());
  std::merge(data.begin(), data.end(), wires.begin(), wires.end(), spans.begin(), span_before);
  Span sw, so;
  if (!(rc = check_overlaps(spans, &sw, &so)) || so.wire) return rc;
  // a stream over a fragment: say which of its entry's fragments (the first that meets the stream)
  for (int i = 0; i < w[so.k].iovcnt; i++) {
    const hdfs_crc32c_iovec &f = w[so.k].iov[i];
    const uintptr_t a = reinterpret_cast<uintptr_t>(f.base);
    if (f.len && a < sw.hi && sw.lo < a + uintptr_t(f.len))
      return fail(rc, "entry %u: wire overlaps fragment %d of entry %u", sw.k, i, so.k);
  }
  return rc;
}

// ---- device state -------------------------------------------------------------
// On the engine's device: the CRC tables and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept;
// the batch's device tables and their pinned staging twin, grown on demand,
// never shrunk, kept between calls.  Calls hold g_mu from the tables' upload
// to the final synchronise, so one call's tables are never overwritten under
// its kernel.
std::mutex g_mu;
using Fused = hdfs_wire_fused::DeviceState<prepare_frame_fused_gather_batch, kBatchMaxGroups>;
struct Scratch : DeviceScratch {
  Fused fused;
  TablePair tab;

  int reserve(int to, size_t tab_bytes) {
    int rc = bind(to, "stream", [this] {
      fused.release();
      tab.release();
    });
    if (rc || (rc = fused.setup(to))) return rc;
    return tab.reserve(tab_bytes, kTableFloor);
  }
} g_s;

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_wirev_fused_batch_compose.  timing: the
// same on the library's stream, then the kernel alone iters more times between
// two events (hdfs_wirev_fused_batch_time).
int compose(hdfs_wirev_fused_batch_write *w, size_t n, int proto, int ctype, hdfs_crc32c_out_packet *pkts,
            size_t max_pkts, size_t *npkts, void *stream, bool timing, unsigned flags, int iters,
            double *ms_per_iter) {
  if (npkts) *npkts = 0;
  if (ms_per_iter) *ms_per_iter = 0;
  Batch B;
  Gather G;
  int rc = layout_batch(w, n, proto, ctype, B, G);
  if (npkts) *npkts = size_t(B.npkts);
  if (rc) return rc;
  const Entry *E = G.E.data();
  const bool fits = pkts && max_pkts >= B.npkts;
  const size_t with_wire = count_wires(E, n);
  if (timing) {  // decided by the arguments alone, before any device is asked
    if (iters < 1 || !ms_per_iter) return fail(HDFS_CRC32C_EINVAL, "iters >= 1 and ms_per_iter are needed");
    if ((rc = Fused::flags_ok(flags))) return rc;
    if (!with_wire) return fail(HDFS_CRC32C_EINVAL, "stream buffers are needed");
  }
  if (!with_wire) {  // size query; the records are closed-form, so they are filled when they fit
    if (fits) fill_batch_records(E, B, pkts);
    return HDFS_CRC32C_OK;
  }
  if ((rc = check_entries(E, n, with_wire, B, pkts, max_pkts))) return rc;
  for (size_t k = 0; k < n; k++)
    for (int i = 0; i < w[k].iovcnt; i++)
      if (w[k].iov[i].len && !w[k].iov[i].base)
        return fail(HDFS_CRC32C_EINVAL, "entry %zu: fragment %d: null base with %llu bytes", k, i,
                    (unsigned long long)w[k].iov[i].len);
  if (!B.npkts) return HDFS_CRC32C_OK;  // nothing but empty writes without finish: no packet
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_gather_places(w, n, G.nfrags, dev))) return rc;
  const bool crcs = ctype != HDFS_CRC32C_CSUM_NULL;
  const uint32_t nw = uint32_t(B.entries), total = uint32_t(B.npkts);
  size_t nfe = 0;  // the fragment table's entries: the fragments and the sentinel of every write that has packets
  for (size_t k = 0; k < n; k++)
    if (!B.L[k].plan.empty()) nfe += size_t(G.nf(k)) + 1;
  const Tables T = tables_of(nw, nfe);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, T.bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  // the tables, in pinned memory: the writes that have packets (the others are
  // dropped here, so the kernel's lookup never meets an empty entry), their
  // fragments slice after slice, and the two prefixes
  uint8_t *base = g_s.tab.pin.as<uint8_t>();
  Frag *ft = reinterpret_cast<Frag *>(base);
  Write *tab = reinterpret_cast<Write *>(base + T.tab);
  uint32_t *pk0 = reinterpret_cast<uint32_t *>(base + T.pk0), *fr0 = reinterpret_cast<uint32_t *>(base + T.fr0);
  uint32_t e = 0, f = 0;
  for (size_t k = 0; k < n; k++) {
    const Layout &L = B.L[k];
    if (L.plan.empty()) continue;
    if (L.w.hb > 31u) return fail(HDFS_CRC32C_EINVAL, "internal: a header of %u bytes", L.w.hb);
    Write &t = tab[e];
    t = L.w;
    t.data = nullptr;  // the data are the fragments': the kernel counts in their concatenation
    t.crc = nullptr;
    t.wire = static_cast<uint8_t *>(w[k].wire);
    pk0[e] = uint32_t(w[k].first_pkt);
    fr0[e++] = f;
    const uint64_t *at = G.at.data() + G.first[k];
    for (int i = 0; i < w[k].iovcnt; i++)
      if (w[k].iov[i].len) ft[f++] = Frag{static_cast<const uint8_t *>(w[k].iov[i].base), *at++};
    ft[f++] = Frag{nullptr, *at};  // the write's sentinel: its length
    if (*at != w[k].len || f - fr0[e - 1] != G.nf(k) + 1u)
      return fail(HDFS_CRC32C_EINVAL, "internal: entry %zu's fragment table does not add up", k);
  }
  pk0[e] = total;
  fr0[e] = f;
  if (e != nw || f != nfe) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's tables do not add up");
  const uint32_t *crc_tab = g_s.fused.tables(ctype);
  const uint32_t groups = g_s.fused.grid(flags, total);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  const hipError_t up = hipMemcpyAsync(g_s.tab.dev.p, g_s.tab.pin.p, T.bytes, hipMemcpyHostToDevice, st);
  // the tables are out of use when this returns, so before the lock goes
  rc = timed_frame_run(st, up, nullptr, g_s.ev, timing ? iters : 0, ms_per_iter, "fused gather wire batch", [&] {
    return launch_frame_fused_gather_batch(g_s.tab.dev.p, nw, uint32_t(nfe), total, uint32_t(proto), crcs, crc_tab,
                                           groups, st);
  });
  if (rc) return rc;
  if (fits) fill_batch_records(E, B, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wirev_fused_batch

using namespace hdfs_wirev_fused_batch;

extern "C" {

int hdfs_wirev_fused_batch_abi_version(void) { return HDFS_WIREV_FUSED_BATCH_ABI_VERSION; }

const char *hdfs_wirev_fused_batch_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_wirev_fused_batch_layout(hdfs_wirev_fused_batch_write *w, size_t nwrites, int proto, int ctype,
                                  hdfs_wirev_fused_batch_totals *out) {
  Gather G;
  RoundCounts c;
  const int rc = layout_totals(out, [&](Batch &B) {
    const int lrc = layout_batch(w, nwrites, proto, ctype, B, G);
    if (lrc) return lrc;
    for (size_t k = 0; k < nwrites; k++) {  // as hdfs_wirev_fused_layout counts each write: the hint starts at 0
      uint32_t hint = 0;
      for (const hdfs_crc32c::outpkt::OutPlan &p : B.L[k].plan)
        if (p.dlen > 0) count_packet(G.at.data() + G.first[k], G.nf(k), p.data_off, uint32_t(p.dlen), hint, c);
    }
    return HDFS_CRC32C_OK;
  });
  if (!out || rc) return rc;
  out->nfrags = G.nfrags;
  out->rounds = c.rounds;
  out->seamed_rounds = c.seamed_rounds;
  out->seamed_ragged = c.seamed_ragged;
  out->max_frags_per_round = c.max_frags_per_round;
  return rc;
}

int hdfs_wirev_fused_batch_compose(hdfs_wirev_fused_batch_write *w, size_t nwrites, int proto, int ctype,
                                   hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, void *stream) {
  return compose(w, nwrites, proto, ctype, pkts, max_pkts, npkts, stream, false, 0u, 0, nullptr);
}

int hdfs_wirev_fused_batch_time(hdfs_wirev_fused_batch_write *w, size_t nwrites, int proto, int ctype,
                                unsigned flags, int iters, double *ms_per_iter) {
  return compose(w, nwrites, proto, ctype, nullptr, 0, nullptr, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
