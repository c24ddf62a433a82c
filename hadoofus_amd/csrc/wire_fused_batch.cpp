// libhadoofus_wire_fused_batch.so: entry points of
// include/hadoofus_wire_fused_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// It asks that library for no CRC: its kernel (frame_fused_batch_kernel)
// computes the chunk CRCs of every write of the batch from the bytes it
// copies, from tables (wire_fused_host.h) built out of crc32c_tables.h.  The
// layout of a write and its records are wire_layout.h's; a batch's front end
// (the entry struct's fields, "entry <k>" in every refusal, where the buffers
// may lie) is wire_batch_layout.h's, shared with the two-pass batch library.
#include <hip/hip_runtime.h>

#include <mutex>

#include "crc32c_outpkt.h"
#include "hadoofus_wire_fused_batch.h"
#include "wire_batch_layout.h"
#include "wire_fused_batch_internal.h"
#include "wire_fused_host.h"
#include "wire_fused_tables.h"
#include "wire_layout.h"

namespace hdfs_wire_fused {
namespace {

using namespace hdfs_wire;  // the layout of a write, its records, the timed run: wire_layout.h's

constexpr uint64_t kMaxPackets = 0x7FFFFFFFull / 4u;  // (2^31 - 1) / 4, the two-pass batch library's limit

// ---- layout of the batch ------------------------------------------------------------
// Fills the out fields of every entry and the totals.  The packet total is
// judged first, in closed form.
int layout_batch(hdfs_wire_fused_batch_write *w, size_t n, int proto, int ctype, Batch &B) {
  Counts c;
  int rc = count_batch(w, n, HDFS_WIRE_FUSED_BATCH_MAX_WRITES, proto, ctype, c);
  if (rc) return rc;
  if (c.packets > kMaxPackets)
    return fail(HDFS_CRC32C_EINVAL, "%llu packets in the batch, at most %llu", (unsigned long long)c.packets,
                (unsigned long long)kMaxPackets);
  if ((rc = layout_entries(w, n, proto, ctype, B))) return rc;
  if (B.npkts != c.packets) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's packet counts do not add up");
  return HDFS_CRC32C_OK;
}

// ---- device state -------------------------------------------------------------
// On the engine's device: the CRC tables and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept;
// the batch's device table and its pinned staging twin, grown on demand,
// never shrunk, kept between calls.  Calls hold
// g_mu from the table's upload to the final synchronise, so one call's table
// is never overwritten under its kernel.
std::mutex g_mu;
using Fused = DeviceState<prepare_frame_fused_batch, kBatchMaxGroups>;
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
  const size_t with_wire = count_wires(w, n);
  if (timing) {  // decided by the arguments alone, before any device is asked
    if (iters < 1 || !ms_per_iter) return fail(HDFS_CRC32C_EINVAL, "iters >= 1 and ms_per_iter are needed");
    if ((rc = Fused::flags_ok(flags))) return rc;
    if (!with_wire) return fail(HDFS_CRC32C_EINVAL, "stream buffers are needed");
  }
  if (!with_wire) {  // size query; the records are closed-form, so they are filled when they fit
    if (fits) fill_batch_records(w, B, pkts);
    return HDFS_CRC32C_OK;
  }
  if ((rc = check_entries(w, n, with_wire, B, pkts, max_pkts))) return rc;
  if (!B.npkts) return HDFS_CRC32C_OK;  // nothing but empty writes without finish: no packet
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_batch_places(w, n, dev))) return rc;
  const bool crcs = ctype != HDFS_CRC32C_CSUM_NULL;
  const uint32_t nw = uint32_t(B.entries), total = uint32_t(B.npkts);
  const size_t tab_bytes = fused_batch_table_bytes(nw);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, tab_bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  // the table, in pinned memory: the writes that have packets (the others are
  // dropped here, so the kernel's lookup never meets an empty entry) and the
  // prefix of their packet counts
  Write *tab = g_s.tab.pin.as<Write>();
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
  const uint32_t *crc_tab = g_s.fused.tables(ctype);
  const uint32_t groups = g_s.fused.grid(flags, total);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  const hipError_t up = hipMemcpyAsync(g_s.tab.dev.p, g_s.tab.pin.p, tab_bytes, hipMemcpyHostToDevice, st);
  // the table is out of use when this returns, so before the lock goes
  rc = timed_frame_run(st, up, nullptr, g_s.ev, timing ? iters : 0, ms_per_iter, "fused wire batch", [&] {
    return launch_frame_fused_batch(g_s.tab.dev.p, nw, total, uint32_t(proto), crcs, crc_tab, groups, st);
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
  return layout_totals(out, [&](Batch &B) { return layout_batch(w, nwrites, proto, ctype, B); });
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
