// libhadoofus_wire_batch.so: entry points of include/hadoofus_wire_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API), the chunk CRCs of every write of
// a batch come from one compute plan of that library, and both share one HIP
// runtime.  The layout of a write and its records are wire_layout.h's, the
// single-write library's own; a batch's front end (every entry's layout, the
// argument checks, where the buffers may lie) is wire_batch_layout.h's, shared
// with the fused batch library; this library's kernel (frame_batch_kernel)
// only moves bytes, with wire_frame.h's code.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "crc32c_outpkt.h"
#include "hadoofus_wire_batch.h"
#include "wire_batch_internal.h"
#include "wire_batch_layout.h"
#include "wire_layout.h"

namespace hdfs_wire {
namespace {

static_assert(kBatchSlices == kSlices, "the batch kernel deals a packet as frame_packets_kernel does");

constexpr uint64_t kMaxPackets = 0x7FFFFFFFull / kBatchSlices;  // the grid: packets * 4 <= 2^31 - 1
constexpr uint64_t kMaxChunks = 0xFFFFFFFFull - 15u;            // 2^32 - 16

// ---- layout of the batch ------------------------------------------------------------
// Fills the out fields of every entry and the totals.  The chunk total is
// judged first, in closed form; the packet total once every entry's out
// fields are set.
int layout_batch(hdfs_wire_batch_write *w, size_t n, int proto, int ctype, Batch &B) {
  Counts c;
  int rc = count_batch(w, n, HDFS_WIRE_BATCH_MAX_WRITES, proto, ctype, c);
  if (rc) return rc;
  if (c.chunks > kMaxChunks)
    return fail(HDFS_CRC32C_EINVAL, "%llu chunks in the batch, at most %llu", (unsigned long long)c.chunks,
                (unsigned long long)kMaxChunks);
  if ((rc = layout_entries(w, n, proto, ctype, B))) return rc;
  if (B.npkts > kMaxPackets)
    return fail(HDFS_CRC32C_EINVAL, "%llu packets in the batch, at most %llu", (unsigned long long)B.npkts,
                (unsigned long long)kMaxPackets);
  if (B.nchunks != c.chunks) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's chunk counts do not add up");
  return HDFS_CRC32C_OK;
}

// ---- device scratch -----------------------------------------------------------
// The CRC array, the device tables and their pinned staging area of one call,
// on the engine's device; grown on demand, never shrunk, kept between calls.
// Calls hold g_mu from the plan to the final synchronise, so one call's CRCs
// and tables are never overwritten under its kernel.
std::mutex g_mu;
struct Scratch : DeviceScratch {
  DeviceBuffer crc;
  TablePair tab;

  int reserve(int to, size_t crc_bytes, size_t tab_bytes) {
    int rc = bind(to, "stream", [this] {
      crc.release();
      tab.release();
    });
    if (rc || (rc = crc.reserve(crc_bytes, kScratchFloor))) return rc;
    return tab.reserve(tab_bytes, kTableFloor);
  }
} g_s;

// ---- the call -------------------------------------------------------------------------
// iters == 0: the call of hdfs_wire_batch_compose.  iters > 0: the same, then
// the frame kernel alone iters more times between two events
// (hdfs_wire_batch_frame_time).
int compose(hdfs_wire_batch_write *w, size_t n, int proto, int ctype, hdfs_crc32c_out_packet *pkts, size_t max_pkts,
            size_t *npkts, void *stream, int iters, double *ms_per_iter) {
  if (npkts) *npkts = 0;
  Batch B;
  int rc = layout_batch(w, n, proto, ctype, B);
  if (npkts) *npkts = size_t(B.npkts);
  if (rc) return rc;
  const bool fits = pkts && max_pkts >= B.npkts;
  const size_t with_wire = count_wires(w, n);
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
  const size_t tab_bytes = batch_table_bytes(nw);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, crcs ? size_t(B.nchunks) * 4 : 0, tab_bytes)) || (iters && (rc = g_s.timing_events())))
    return rc;
  // the tables, in pinned memory: the writes that have packets (the others are
  // dropped here, so the kernel's search never meets an empty entry) and the
  // prefix of their packet counts; the CRCs: every write's chunk grid as
  // segments of one compute plan, write k's CRCs behind those of the writes
  // ahead of it
  Write *tab = g_s.tab.pin.as<Write>();
  uint32_t *pk0 = reinterpret_cast<uint32_t *>(tab + nw);
  std::vector<hdfs_crc32c_segment> segs;
  if (crcs) segs.reserve(2 * size_t(nw));
  hdfs_crc32c_segment two[2];
  uint64_t c0 = 0;
  uint32_t e = 0;
  for (size_t k = 0; k < n; k++) {
    const Layout &L = B.L[k];
    if (L.plan.empty()) continue;
    Write &t = tab[e];
    t = L.w;
    t.slices = kBatchSlices;
    t.data = static_cast<const uint8_t *>(w[k].data);
    t.crc = g_s.crc.as<uint32_t>() + c0;
    t.wire = static_cast<uint8_t *>(w[k].wire);
    pk0[e++] = uint32_t(w[k].first_pkt);
    if (crcs && t.len) {
      segs.insert(segs.end(), two, two + grid_segments(t, g_s.crc.as<uint32_t>() + c0, ctype, two));
      c0 += L.nchunks;
    }
  }
  pk0[e] = total;
  if (e != nw || c0 > B.nchunks) return fail(HDFS_CRC32C_EINVAL, "internal: the batch's tables do not add up");
  hdfs_crc32c_plan *cplan = nullptr;
  if (!segs.empty() && (rc = hdfs_crc32c_plan_create(&cplan, HDFS_CRC32C_MODE_COMPUTE, segs.data(), segs.size())))
    return engine_fail(rc, "compute plan");
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  const hipError_t up = hipMemcpyAsync(g_s.tab.dev.p, g_s.tab.pin.p, tab_bytes, hipMemcpyHostToDevice, st);
  // the CRC array and the tables are out of use when this returns, so before the lock goes
  rc = timed_frame_run(st, up, cplan, g_s.ev, iters, ms_per_iter, "wire batch",
                       [&] { return launch_frame_batch(g_s.tab.dev.p, nw, total, st); });
  if (rc) return rc;
  if (fits) fill_batch_records(w, B, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wire

using namespace hdfs_wire;

extern "C" {

int hdfs_wire_batch_abi_version(void) { return HDFS_WIRE_BATCH_ABI_VERSION; }

const char *hdfs_wire_batch_last_error(void) { return last_error(); }

int hdfs_wire_batch_layout(hdfs_wire_batch_write *w, size_t nwrites, int proto, int ctype,
                           hdfs_wire_batch_totals *out) {
  return layout_totals(out, [&](Batch &B) { return layout_batch(w, nwrites, proto, ctype, B); });
}

int hdfs_wire_batch_compose(hdfs_wire_batch_write *w, size_t nwrites, int proto, int ctype,
                            hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, void *stream) {
  return compose(w, nwrites, proto, ctype, pkts, max_pkts, npkts, stream, 0, nullptr);
}

int hdfs_wire_batch_frame_time(hdfs_wire_batch_write *w, size_t nwrites, int proto, int ctype, int iters,
                               double *ms_per_iter) {
  if (iters < 1 || !ms_per_iter) return fail(HDFS_CRC32C_EINVAL, "iters >= 1 and ms_per_iter are needed");
  *ms_per_iter = 0;
  const size_t listed = std::min(nwrites, size_t(HDFS_WIRE_BATCH_MAX_WRITES));  // a longer list is compose's to refuse
  if (!w || !count_wires(w, listed)) return fail(HDFS_CRC32C_EINVAL, "stream buffers are needed");
  return compose(w, nwrites, proto, ctype, nullptr, 0, nullptr, nullptr, iters, ms_per_iter);
}

}  // extern "C"
