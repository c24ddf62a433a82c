// libhadoofus_wire_fused.so: entry points of include/hadoofus_wire_fused.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Unlike libhadoofus_wire.so it asks that library for no CRC: its own kernel
// (frame_fused_kernel) computes the chunk CRCs from the bytes it copies, from
// tables (wire_fused_host.h) built out of crc32c_tables.h.
#include <hip/hip_runtime.h>

#include <mutex>

#include "crc32c_outpkt.h"
#include "hadoofus_wire_fused.h"
#include "wire_fused_host.h"
#include "wire_fused_internal.h"
#include "wire_fused_tables.h"
#include "wire_layout.h"

namespace hdfs_wire_fused {
namespace {

using namespace hdfs_wire;  // the layout of a write, its records, the timed run: wire_layout.h's

// ---- device state -------------------------------------------------------------
// The CRC tables on the engine's device and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept.
// Calls hold g_mu from the launch to the final synchronise.
std::mutex g_mu;
using Fused = DeviceState<prepare_frame_fused, kMaxGroups>;
struct Scratch : DeviceScratch {
  Fused fused;

  int reserve(int to) {
    const int rc = bind(to, "stream", [this] { fused.release(); });
    return rc ? rc : fused.setup(to);
  }
} g_s;

// ---- the call -------------------------------------------------------------------------
// iters == 0: the call of hdfs_wire_fused_compose_packets.  iters > 0: the
// same, then the kernel alone iters more times between two events
// (hdfs_wire_fused_time).
int compose(const void *data, uint64_t len, int64_t off, int64_t seq, int proto, int ctype, int finish, void *wire,
            uint64_t wire_cap, hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, uint64_t *wire_len,
            void *stream, unsigned flags, int iters, double *ms_per_iter) {
  if (npkts) *npkts = 0;
  if (wire_len) *wire_len = 0;
  if (!args_ok(proto, ctype, off, len)) return HDFS_CRC32C_EINVAL;
  Layout L;
  int rc = build_layout(len, off, seq, proto, ctype, finish != 0, L);
  if (rc) return rc;
  if (npkts) *npkts = L.plan.size();
  if (wire_len) *wire_len = L.wire_len;
  const bool fits = pkts && max_pkts >= L.plan.size();
  if (!wire) {  // size query; the records are closed-form, so they are filled when they fit
    if (fits) fill_records(L, pkts);
    return HDFS_CRC32C_OK;
  }
  if (len && !data) return fail(HDFS_CRC32C_EINVAL, "null data with %llu bytes", (unsigned long long)len);
  if ((pkts && !fits) || wire_cap < L.wire_len)
    return fail(HDFS_CRC32C_EINVAL, "need %zu packets / %llu stream bytes", L.plan.size(), (unsigned long long)L.wire_len);
  if ((rc = Fused::flags_ok(flags))) return rc;
  if (!L.wire_len) return HDFS_CRC32C_OK;  // an empty write without finish: no packet
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if (len && (rc = device_range(data, len, dev, "data"))) return rc;
  if ((rc = device_range(wire, L.wire_len, dev, "wire"))) return rc;
  const uintptr_t a = reinterpret_cast<uintptr_t>(data), b = reinterpret_cast<uintptr_t>(wire);
  if (len && a < b + L.wire_len && b < a + len) return fail(HDFS_CRC32C_EINVAL, "data and wire overlap");
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev)) || (iters && (rc = g_s.timing_events()))) return rc;
  Write w = L.w;
  w.data = static_cast<const uint8_t *>(data);
  w.crc = nullptr;
  w.wire = static_cast<uint8_t *>(wire);
  const uint32_t *tab = g_s.fused.tables(ctype);
  const uint32_t groups = g_s.fused.grid(flags, w.npk);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  rc = timed_frame_run(st, hipSuccess, nullptr, g_s.ev, iters, ms_per_iter, "fused wire stream",
                       [&] { return launch_frame_fused(w, tab, groups, st); });
  if (rc) return rc;
  if (fits) fill_records(L, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wire_fused

using namespace hdfs_wire_fused;

extern "C" {

int hdfs_wire_fused_abi_version(void) { return HDFS_WIRE_FUSED_ABI_VERSION; }

const char *hdfs_wire_fused_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_wire_fused_compose_packets(const void *data, uint64_t len, int64_t offset_in_block, int64_t seqno, int proto,
                                    int ctype, int finish, void *wire, uint64_t wire_cap,
                                    hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, uint64_t *wire_len,
                                    void *stream) {
  return compose(data, len, offset_in_block, seqno, proto, ctype, finish, wire, wire_cap, pkts, max_pkts, npkts,
                 wire_len, stream, 0u, 0, nullptr);
}

int hdfs_wire_fused_time(const void *data, uint64_t len, int64_t offset_in_block, int proto, int ctype, int finish,
                         void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter) {
  if (iters < 1 || !ms_per_iter || !wire)
    return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "iters >= 1, a stream buffer and ms_per_iter are needed");
  return compose(data, len, offset_in_block, 0, proto, ctype, finish, wire, wire_cap, nullptr, 0, nullptr, nullptr,
                 nullptr, flags, iters, ms_per_iter);
}

}  // extern "C"
