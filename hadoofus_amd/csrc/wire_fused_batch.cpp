// libhadoofus_wire_fused_batch.so: entry points of
// include/hadoofus_wire_fused_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// It asks that library for no CRC: its kernel (frame_fused_batch_kernel)
// computes the chunk CRCs of every write of the batch from the bytes it
// copies, from tables built here out of crc32c_tables.h.  The layout of a
// write and its records are wire_layout.h's; the conventions of a batch (the
// entry struct, "entry <k>" in every refusal, writes without packets dropped
// here) are the two-pass batch library's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "crc32c_outpkt.h"
#include "hadoofus_wire_fused_batch.h"
#include "wire_fused_batch_internal.h"
#include "wire_fused_tables.h"
#include "wire_layout.h"

namespace hdfs_wire_fused {
namespace {

using namespace hdfs_wire;  // the layout of a write, its records, the timed run: wire_layout.h's

constexpr uint64_t kMaxPackets = 0x7FFFFFFFull / 4u;  // (2^31 - 1) / 4, the two-pass batch library's limit
constexpr size_t kTableFloor = size_t(16) << 10;

// The failure just recorded (by the shared layout code) was entry k's.
int entry_fail(int rc, size_t k) { return prefix_fail(rc, "entry %zu", k); }

// ---- layout of the batch ------------------------------------------------------------
struct Batch {
  std::vector<Layout> L;  // per entry
  uint64_t npkts = 0, nchunks = 0, wire_bytes = 0, entries = 0;
};

// Fills the out fields of every entry and the totals.
int layout_batch(hdfs_wire_fused_batch_write *w, size_t n, int proto, int ctype, Batch &B) {
  if (n > HDFS_WIRE_FUSED_BATCH_MAX_WRITES)
    return fail(HDFS_CRC32C_EINVAL, "%zu writes, at most %d in one call", n, HDFS_WIRE_FUSED_BATCH_MAX_WRITES);
  if (n && !w) return fail(HDFS_CRC32C_EINVAL, "null writes");
  for (size_t k = 0; k < n; k++) w[k].wire_len = w[k].npkts = w[k].first_pkt = 0;
  // the arguments and the packet total first, in closed form: a batch past the
  // limit is refused before any write's packets are walked
  uint64_t packets = 0;
  for (size_t k = 0; k < n; k++) {
    if (!args_ok(proto, ctype, w[k].offset_in_block, w[k].len)) return entry_fail(HDFS_CRC32C_EINVAL, k);
    const uint64_t mis = uint64_t(w[k].offset_in_block) % kChunk, to_grid = mis ? kChunk - mis : 0u;
    const uint64_t n0 = std::min(w[k].len, to_grid);
    packets += (n0 ? 1u : 0u) + (w[k].len - n0 + kPacket - 1) / kPacket + (w[k].finish ? 1u : 0u);
  }
  if (packets > kMaxPackets)
    return fail(HDFS_CRC32C_EINVAL, "%llu packets in the batch, at most %llu", (unsigned long long)packets,
                (unsigned long long)kMaxPackets);
  B.L.resize(n);
  for (size_t k = 0; k < n; k++) {
    Layout &L = B.L[k];
    const int rc = build_layout(w[k].len, w[k].offset_in_block, w[k].seqno, proto, ctype, w[k].finish != 0, L);
    if (rc) return entry_fail(rc, k);
    w[k].wire_len = L.wire_len;
    w[k].npkts = L.plan.size();
    w[k].first_pkt = B.npkts;
    B.npkts += L.plan.size();
    B.nchunks += L.nchunks;
    B.wire_bytes += L.wire_len;
    B.entries += L.plan.empty() ? 0u : 1u;
  }
  if (B.npkts != packets) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's packet counts do not add up");
  return HDFS_CRC32C_OK;
}

void fill_batch_records(const hdfs_wire_fused_batch_write *w, const Batch &B, hdfs_crc32c_out_packet *pkts) {
  for (size_t k = 0; k < B.L.size(); k++) fill_records(B.L[k], pkts + w[k].first_pkt);
}

// ---- device state -------------------------------------------------------------
// On the engine's device: the compact CRC tables of both polynomials (CRC32C
// first), uploaded when the library is first used there and kept; the batch's
// device table and its pinned staging area, grown on demand, never shrunk,
// kept between calls; the workgroups of one launch, one per CU.  Calls hold
// g_mu from the table's upload to the final synchronise, so one call's table
// is never overwritten under its kernel.
std::mutex g_mu;
struct Scratch : DeviceScratch {
  DeviceBuffer crc_tab, tab;
  PinnedBuffer<> pin;  // the table's staging area: tab's twin, grown with it
  bool ready = false;
  uint32_t groups = 0;
  hipEvent_t ev[2] = {nullptr, nullptr};  // of the timing call, created when it first runs

  int reserve(int to, size_t tab_bytes) {
    int rc = bind(to, "stream", [this] {
      crc_tab.release();
      tab.release();
      pin.release();
      ready = false;
      for (hipEvent_t &e : ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
      }
    });
    if (rc) return rc;
    if (!ready) {
      std::vector<uint32_t> host(2 * crc::kCompactWords);
      crc::make_compact(hdfs_crc32c::kPoly, host.data());
      crc::make_compact(hdfs_crc32c::kPolyZlib, host.data() + crc::kCompactWords);
      if ((rc = crc_tab.reserve(host.size() * sizeof(uint32_t), 0))) return rc;
      int cus = 0;
      hipError_t e = hipMemcpy(crc_tab.p, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, to);
      if (e == hipSuccess) e = prepare_frame_fused_batch();
      if (e != hipSuccess) return fail(HDFS_CRC32C_EHIP, "tables: %s", hipGetErrorString(e));
      groups = cus < 1 ? 1u : (uint32_t(cus) > kBatchMaxGroups ? kBatchMaxGroups : uint32_t(cus));
      ready = true;
    }
    if (tab_bytes <= tab.cap) return HDFS_CRC32C_OK;
    tab.release();  // both go before either comes back
    pin.release();
    if (tab.reserve(tab_bytes, kTableFloor) || pin.reserve(tab_bytes, kTableFloor)) {
      tab.release();
      return fail(HDFS_CRC32C_ENOMEM, "allocation of %zu table bytes failed", std::max(tab_bytes, kTableFloor));
    }
    return HDFS_CRC32C_OK;
  }
  int timing_events() {
    if (!ev[0] && (hipEventCreate(&ev[0]) != hipSuccess || hipEventCreate(&ev[1]) != hipSuccess))
      return fail(HDFS_CRC32C_EHIP, "events: %s", hipGetErrorString(hipGetLastError()));
    return HDFS_CRC32C_OK;
  }
} g_s;

// ---- where the buffers live -------------------------------------------------------
// No wire range overlaps another wire range or a data range: the intervals
// sorted by their first byte, then one pass that remembers the furthest end
// among the wire ranges and among the data ranges seen so far (as the
// two-pass batch library checks it).
struct Span {
  uintptr_t lo, hi;  // [lo, hi), not empty
  uint32_t k;        // entry
  uint32_t wire;     // 1: a wire range
};

int check_overlaps(std::vector<Span> &v) {
  std::sort(v.begin(), v.end(), [](const Span &a, const Span &b) {
    return a.lo != b.lo ? a.lo < b.lo : (a.wire != b.wire ? a.wire > b.wire : a.k < b.k);
  });
  const Span *far_w = nullptr, *far_d = nullptr;
  for (const Span &s : v) {
    // every span ahead of s starts at or below s.lo: it overlaps s iff it ends behind s.lo
    if (far_w && far_w->hi > s.lo) {
      const uint32_t a = std::max(far_w->k, s.k), b = std::min(far_w->k, s.k);
      return s.wire ? fail(HDFS_CRC32C_EINVAL, "entry %u: wire overlaps the wire of entry %u", a, b)
                    : fail(HDFS_CRC32C_EINVAL, "entry %u: wire overlaps the data of entry %u", far_w->k, s.k);
    }
    if (s.wire && far_d && far_d->hi > s.lo)
      return fail(HDFS_CRC32C_EINVAL, "entry %u: wire overlaps the data of entry %u", s.k, far_d->k);
    const Span *&far = s.wire ? far_w : far_d;
    if (!far || s.hi > far->hi) far = &s;
  }
  return HDFS_CRC32C_OK;
}

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_wire_fused_batch_compose.  timing: the
// same on the library's stream, then the kernel alone iters more times between
// two events (hdfs_wire_fused_batch_time).
int compose(hdfs_wire_fused_batch_write *w, size_t n, int proto, int ctype, hdfs_crc32c_out_packet *pkts,
            size_t max_pkts, size_t *npkts, void *stream, bool timing, unsigned flags, int iters,
            double *ms_per_iter) {
  if (npkts) *npkts = 0;
  if (ms_per_iter) *ms_per_iter = 0;
  Batch B;
  int rc = layout_batch(w, n, proto, ctype, B);
  if (npkts) *npkts = size_t(B.npkts);
  if (rc) return rc;
  const bool fits = pkts && max_pkts >= B.npkts;
  size_t with_wire = 0;
  for (size_t k = 0; k < n; k++) with_wire += w[k].wire ? 1u : 0u;
  const unsigned want = flags >> 8;
  if (timing) {  // decided by the arguments alone, before any device is asked
    if (iters < 1 || !ms_per_iter) return fail(HDFS_CRC32C_EINVAL, "iters >= 1 and ms_per_iter are needed");
    if ((flags & 0xFFu) || want > kBatchMaxGroups)
      return fail(HDFS_CRC32C_EINVAL, "1 to %u workgroups", kBatchMaxGroups);
    if (!with_wire) return fail(HDFS_CRC32C_EINVAL, "stream buffers are needed");
  }
  if (!with_wire) {  // size query; the records are closed-form, so they are filled when they fit
    if (fits) fill_batch_records(w, B, pkts);
    return HDFS_CRC32C_OK;
  }
  if (with_wire != n) {
    const bool first = w[0].wire != nullptr;
    size_t k = 1;
    while ((w[k].wire != nullptr) == first) k++;
    return fail(HDFS_CRC32C_EINVAL, "entry %zu: wire is %s, entry 0's is not (every wire NULL is a size query)", k,
                first ? "NULL" : "set");
  }
  for (size_t k = 0; k < n; k++) {
    if (w[k].len && !w[k].data)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: null data with %llu bytes", k, (unsigned long long)w[k].len);
    if (w[k].wire_cap < w[k].wire_len)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: %llu stream bytes, room for %llu", k,
                  (unsigned long long)w[k].wire_len, (unsigned long long)w[k].wire_cap);
    if (pkts && w[k].first_pkt + w[k].npkts > max_pkts)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: its records end at %llu of %llu, room for %zu", k,
                  (unsigned long long)(w[k].first_pkt + w[k].npkts), (unsigned long long)B.npkts, max_pkts);
  }
  if (!B.npkts) return HDFS_CRC32C_OK;  // nothing but empty writes without finish: no packet
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  {
    Allocations al;
    std::vector<Span> spans;
    spans.reserve(2 * n);
    for (size_t k = 0; k < n; k++) {
      const uintptr_t a = reinterpret_cast<uintptr_t>(w[k].data), b = reinterpret_cast<uintptr_t>(w[k].wire);
      if (w[k].len) {
        if ((rc = al.check(w[k].data, w[k].len, dev, "data"))) return entry_fail(rc, k);
        spans.push_back(Span{a, a + uintptr_t(w[k].len), uint32_t(k), 0u});
      }
      if (w[k].wire_len) {
        if ((rc = al.check(w[k].wire, w[k].wire_len, dev, "wire"))) return entry_fail(rc, k);
        spans.push_back(Span{b, b + uintptr_t(w[k].wire_len), uint32_t(k), 1u});
      }
    }
    if ((rc = check_overlaps(spans))) return rc;
  }
  const bool crcs = ctype != HDFS_CRC32C_CSUM_NULL;
  const uint32_t nw = uint32_t(B.entries), total = uint32_t(B.npkts);
  const size_t tab_bytes = fused_batch_table_bytes(nw);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, tab_bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  // the table, in pinned memory: the writes that have packets (the others are
  // dropped here, so the kernel's lookup never meets an empty entry) and the
  // prefix of their packet counts
  Write *tab = g_s.pin.as<Write>();
  uint32_t *pk0 = reinterpret_cast<uint32_t *>(tab + nw);
  uint32_t e = 0;
  for (size_t k = 0; k < n; k++) {
    const Layout &L = B.L[k];
    if (L.plan.empty()) continue;
    if (L.w.hb > 31u) return fail(HDFS_CRC32C_EINVAL, "internal: a header of %u bytes", L.w.hb);
    Write &t = tab[e];
    t = L.w;
    t.data = static_cast<const uint8_t *>(w[k].data);
    t.crc = nullptr;
    t.wire = static_cast<uint8_t *>(w[k].wire);
    pk0[e++] = uint32_t(w[k].first_pkt);
  }
  pk0[e] = total;
  if (e != nw) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's tables do not add up");
  const uint32_t *crc_tab =
      g_s.crc_tab.as<uint32_t>() + (ctype == HDFS_CRC32C_CSUM_CRC32 ? crc::kCompactWords : 0u);
  // the product's grid: a workgroup per CU, and none without a packet
  const uint32_t groups = want ? want : std::min(total, g_s.groups);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  const hipError_t up = hipMemcpyAsync(g_s.tab.p, g_s.pin.p, tab_bytes, hipMemcpyHostToDevice, st);
  // the table is out of use when this returns, so before the lock goes
  rc = timed_frame_run(st, up, nullptr, g_s.ev, timing ? iters : 0, ms_per_iter, "fused wire batch", [&] {
    return launch_frame_fused_batch(g_s.tab.p, nw, total, uint32_t(proto), crcs, crc_tab, groups, st);
  });
  if (rc) return rc;
  if (fits) fill_batch_records(w, B, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wire_fused

using namespace hdfs_wire_fused;

extern "C" {

int hdfs_wire_fused_batch_abi_version(void) { return HDFS_WIRE_FUSED_BATCH_ABI_VERSION; }

const char *hdfs_wire_fused_batch_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_wire_fused_batch_layout(hdfs_wire_fused_batch_write *w, size_t nwrites, int proto, int ctype,
                                 hdfs_wire_fused_batch_totals *out) {
  if (!out) return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "null out");
  std::memset(out, 0, sizeof(*out));
  Batch B;
  const int rc = layout_batch(w, nwrites, proto, ctype, B);
  out->npkts = B.npkts;
  out->nchunks = B.nchunks;
  out->wire_bytes = B.wire_bytes;
  out->table_entries = B.entries;
  return rc;
}

int hdfs_wire_fused_batch_compose(hdfs_wire_fused_batch_write *w, size_t nwrites, int proto, int ctype,
                                  hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, void *stream) {
  return compose(w, nwrites, proto, ctype, pkts, max_pkts, npkts, stream, false, 0u, 0, nullptr);
}

int hdfs_wire_fused_batch_time(hdfs_wire_fused_batch_write *w, size_t nwrites, int proto, int ctype, unsigned flags,
                               int iters, double *ms_per_iter) {
  return compose(w, nwrites, proto, ctype, nullptr, 0, nullptr, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
