// libhadoofus_wire.so: entry points of include/hadoofus_wire.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API), the chunk CRCs of a write come
// from one compute plan of that library, and both share one HIP runtime.
// This library's own kernel (frame_packets_kernel) only moves bytes.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "crc32c_outpkt.h"
#include "hadoofus_wire.h"
#include "wire_internal.h"
#include "wire_layout.h"

namespace hdfs_wire {
namespace {

using namespace hdfs_crc32c::outpkt;

// The store policy of the 16-B stores, as measured (tools/wire_bench.py,
// DESIGN.md section 13): plain stores beat write-through ones at every size.
// Workgroups per packet: kSlices (wire_layout.h).
constexpr bool kSc1Stores = false;

// The layout of a write (Layout, args_ok, build_layout), its records
// (fill_records), its plan segments (grid_segments) and the frame run
// (timed_frame_run) are wire_layout.h's, shared with the batch library; the
// last-error text, the scratch base and the check of a buffer's place
// (device_range) are companion_support.h's.

// ---- device scratch -----------------------------------------------------------
// The CRC array of one call, on the engine's device; grown on demand, never
// shrunk, kept between calls.  Calls hold g_mu from the plan to the final
// synchronise, so one call's CRCs are never overwritten under its kernel.
std::mutex g_mu;
struct Scratch : DeviceScratch {
  DeviceBuffer crc;

  int reserve(int to, size_t crc_bytes) {
    const int rc = bind(to, "stream", [this] { crc.release(); });
    return rc ? rc : crc.reserve(crc_bytes, kScratchFloor);
  }
} g_s;

// ---- the call -------------------------------------------------------------------------
// iters == 0: the call of hdfs_wire_compose_packets.  iters > 0: the same,
// then the frame kernel alone iters more times between two events
// (hdfs_wire_frame_time).
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
  if (!L.wire_len) return HDFS_CRC32C_OK;  // an empty write without finish: no packet
  Write w = L.w;
  const unsigned sl = (flags >> 8) & 0xFFu;
  if (sl > kMaxSlices) return fail(HDFS_CRC32C_EINVAL, "at most %u workgroups per packet", kMaxSlices);
  if (sl) w.slices = sl;
  const bool sc1 = iters ? (flags & HDFS_WIRE_TIME_SC1) != 0 : kSc1Stores;
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if (len && (rc = device_range(data, len, dev, "data"))) return rc;
  if ((rc = device_range(wire, L.wire_len, dev, "wire"))) return rc;
  const uintptr_t a = reinterpret_cast<uintptr_t>(data), b = reinterpret_cast<uintptr_t>(wire);
  if (len && a < b + L.wire_len && b < a + len) return fail(HDFS_CRC32C_EINVAL, "data and wire overlap");
  const bool crcs = w.csum && len;
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, crcs ? size_t(L.nchunks) * 4 : 0)) || (iters && (rc = g_s.timing_events()))) return rc;
  w.data = static_cast<const uint8_t *>(data);
  w.crc = g_s.crc.as<uint32_t>();
  w.wire = static_cast<uint8_t *>(wire);
  // the CRCs: one compute plan over the write's chunk grid
  hdfs_crc32c_plan *cplan = nullptr;
  hdfs_crc32c_segment segs[2];
  const size_t ns = grid_segments(w, g_s.crc.as<uint32_t>(), ctype, segs);
  if (ns && (rc = hdfs_crc32c_plan_create(&cplan, HDFS_CRC32C_MODE_COMPUTE, segs, ns))) return engine_fail(rc, "compute plan");
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  // the CRC array is out of use when this returns, so before the lock goes
  rc = timed_frame_run(st, hipSuccess, cplan, g_s.ev, iters, ms_per_iter, "wire stream",
                       [&] { return launch_frame_packets(w, sc1, st); });
  if (rc) return rc;
  if (fits) fill_records(L, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wire

using namespace hdfs_wire;

extern "C" {

int hdfs_wire_abi_version(void) { return HDFS_WIRE_ABI_VERSION; }

const char *hdfs_wire_last_error(void) { return last_error(); }

int hdfs_wire_layout(uint64_t len, int64_t offset_in_block, int proto, int ctype, int finish,
                     hdfs_wire_layout_info *out) {
  if (!out) return fail(HDFS_CRC32C_EINVAL, "null out");
  if (!args_ok(proto, ctype, offset_in_block, len)) return HDFS_CRC32C_EINVAL;
  Layout L;
  const int rc = build_layout(len, offset_in_block, 0, proto, ctype, finish != 0, L);
  if (rc) return rc;
  std::memset(out, 0, sizeof(*out));
  out->npkts = L.plan.size();
  out->nchunks = L.nchunks;
  out->wire_len = L.wire_len;
  out->packet_stride = L.w.hb + (L.w.csum ? 4u * (kPacket / kChunk) : 0u) + kPacket;
  out->header_bytes = L.w.hb;
  out->head_bytes = L.w.n0;
  return HDFS_CRC32C_OK;
}

int hdfs_wire_compose_packets(const void *data, uint64_t len, int64_t offset_in_block, int64_t seqno, int proto,
                              int ctype, int finish, void *wire, uint64_t wire_cap, hdfs_crc32c_out_packet *pkts,
                              size_t max_pkts, size_t *npkts, uint64_t *wire_len, void *stream) {
  return compose(data, len, offset_in_block, seqno, proto, ctype, finish, wire, wire_cap, pkts, max_pkts, npkts,
                 wire_len, stream, 0u, 0, nullptr);
}

int hdfs_wire_frame_time(const void *data, uint64_t len, int64_t offset_in_block, int proto, int ctype, int finish,
                         void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter) {
  if (iters < 1 || !ms_per_iter || !wire) return fail(HDFS_CRC32C_EINVAL, "iters >= 1, a stream buffer and ms_per_iter are needed");
  return compose(data, len, offset_in_block, 0, proto, ctype, finish, wire, wire_cap, nullptr, 0, nullptr, nullptr,
                 nullptr, flags, iters, ms_per_iter);
}

}  // extern "C"
