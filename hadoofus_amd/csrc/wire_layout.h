// Host side shared by the seven wire-stream libraries (wire.cpp, wire_batch.cpp,
// wirev.cpp, wire_fused.cpp, wire_fused_batch.cpp, wirev_fused.cpp,
// wirev_fused_batch.cpp): the
// layout of one write's stream, its packet records, the compute-plan segments
// of its chunk grid (the two-pass libraries') and the timed frame run.  One
// definition, included by all.  What every companion library shares (last
// error, DeviceGuard, device_range, ...) is companion_support.h's; what only
// the batch libraries share is wire_batch_layout.h's, what only the fused
// ones share wire_fused_host.h's.
#ifndef HADOOFUS_WIRE_LAYOUT_H
#define HADOOFUS_WIRE_LAYOUT_H

#include <cstring>
#include <vector>

#include "companion_support.h"
#include "crc32c_outpkt.h"
#include "hadoofus_crc32c.h"
#include "wire_internal.h"

namespace hdfs_wire {

using namespace hdfs_companion;

static_assert(kChunk == hdfs_crc32c::outpkt::kWriteChunk && int64_t(kPacket) == hdfs_crc32c::outpkt::kPacketSize,
              "one packet geometry");

// Workgroups per packet, as measured (tools/wire_bench.py, DESIGN.md section
// 13): four per packet are fastest or within 4 % of the fastest from 1 MiB to
// 1 GiB.
constexpr uint32_t kSlices = 4;

// ---- layout -------------------------------------------------------------------
struct Layout {
  Write w;  // pointers not set
  uint64_t nchunks = 0, wire_len = 0;
  std::vector<hdfs_crc32c::outpkt::OutPlan> plan;
};

inline bool args_ok(int proto, int ctype, int64_t offset_in_block, uint64_t len) {
  if (!packet_args_ok(proto, ctype, offset_in_block)) return false;
  if (len > (uint64_t(1) << 40)) return fail(HDFS_CRC32C_EINVAL, "more than 1 TiB in one write"), false;
  return true;
}

// Packet sizing is outpkt::plan_out_packets', the definition; the kernel's
// closed form (packet_at) is checked against it packet by packet.
inline int build_layout(uint64_t len, int64_t off, int64_t seq, int proto, int ctype, bool finish, Layout &L) {
  using namespace hdfs_crc32c::outpkt;
  plan_out_packets(len, off, seq, finish, L.plan);
  Write &w = L.w;
  std::memset(&w, 0, sizeof(w));
  w.len = len;
  w.off = off;
  w.seq = seq;
  w.n0 = uint32_t(out_head_bytes(L.plan, len, off));
  w.npk = uint32_t(L.plan.size());
  w.hb = out_header_bytes(proto);
  w.proto = uint32_t(proto);
  w.csum = ctype != HDFS_CRC32C_CSUM_NULL ? 1u : 0u;
  w.finish = finish ? 1u : 0u;
  w.slices = kSlices;
  const uint32_t k0 = w.n0 ? 1u : 0u;
  L.nchunks = k0 + (len - w.n0 + kChunk - 1) / kChunk;
  uint64_t pos = 0;
  for (size_t i = 0; i < L.plan.size(); i++) {
    const OutPlan &k = L.plan[i];
    const Pkt p = packet_at(w, uint32_t(i));
    const uint64_t cidx = i < k0 ? 0u : k0 + (k.data_off - w.n0) / kChunk;  // as write_out_packets finds its CRCs
    if (p.wire_off != pos || p.data_off != k.data_off || p.off != k.offset || p.seq != k.seqno ||
        int32_t(p.dlen) != k.dlen || (p.last != 0u) != k.last || (p.ncrc && p.cidx != cidx) ||
        p.cidx + uint64_t(p.ncrc) > L.nchunks)
      return fail(HDFS_CRC32C_EINVAL, "internal: packet %zu of the write is not where its index puts it", i);
    pos += w.hb + 4u * p.ncrc + p.dlen;
  }
  L.wire_len = pos;
  return HDFS_CRC32C_OK;
}

// The packet records: hdfs_crc32c_compose_packets', hdr_off counting in the stream.
inline void fill_records(const Layout &L, hdfs_crc32c_out_packet *pkts) {
  using namespace hdfs_crc32c::outpkt;
  for (size_t i = 0; i < L.plan.size(); i++) {
    const OutPlan &k = L.plan[i];
    const Pkt p = packet_at(L.w, uint32_t(i));
    hdfs_crc32c_out_packet &o = pkts[i];
    std::memset(&o, 0, sizeof(o));
    o.hdr_off = p.wire_off;
    o.data_off = k.data_off;
    o.offset_in_block = k.offset;
    o.seqno = k.seqno;
    o.data_len = k.dlen;
    o.hdr_len = L.w.hb + 4u * p.ncrc;
    o.crc_len = 4u * p.ncrc;
    o.last = k.last ? 1 : 0;
  }
}

// ---- the CRCs of a write ---------------------------------------------------------
// compose_packets' chunk grid of write t as segments of a compute plan: the
// short first chunk, then the 512-B grid behind it; chunk i's CRC goes to
// crc[i].  out has room for two.  -> segments written (none without checksums
// or data).
inline size_t grid_segments(const Write &t, uint32_t *crc, int ctype, hdfs_crc32c_segment *out) {
  if (ctype == HDFS_CRC32C_CSUM_NULL || !t.len) return 0;
  const uint32_t sf = HDFS_CRC32C_SEG_BE | (ctype == HDFS_CRC32C_CSUM_CRC32 ? HDFS_CRC32C_SEG_CRC32 : 0u);
  size_t ns = 0;
  if (t.n0) out[ns++] = hdfs_crc32c_segment{t.data, t.n0, kChunk, sf, 0u, 0u, crc, nullptr};
  if (t.len > t.n0)
    out[ns++] = hdfs_crc32c_segment{t.data + t.n0, t.len - t.n0, kChunk, sf, 0u, 0u, crc + (t.n0 ? 1 : 0), nullptr};
  return ns;
}

// ---- the frame run ------------------------------------------------------------------
// On stream st, after whatever the caller enqueued with status e: the compute
// plan (may be NULL), then launch() once.  iters > 0: then launch() iters more
// times between the two events, and *ms_per_iter is one launch's time.  Always
// synchronises and destroys the plan (sync_and_report).
template <class Launch>
int timed_frame_run(hipStream_t st, hipError_t e, hdfs_crc32c_plan *cplan, hipEvent_t *ev, int iters,
                    double *ms_per_iter, const char *what, Launch launch) {
  int rc = HDFS_CRC32C_OK;
  if (e == hipSuccess && cplan && (rc = hdfs_crc32c_plan_execute(cplan, st))) rc = engine_fail(rc, "compute plan");
  if (!rc && e == hipSuccess) e = launch();
  if (!rc && e == hipSuccess && iters) {
    e = hipEventRecord(ev[0], st);
    for (int i = 0; i < iters && e == hipSuccess; i++) e = launch();
    if (e == hipSuccess) e = hipEventRecord(ev[1], st);
  }
  if ((rc = sync_and_report(st, e, rc, cplan, what)) || !iters) return rc;
  float ms = 0;
  e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  if (ms_per_iter) *ms_per_iter = double(ms) / iters;
  return e == hipSuccess ? HDFS_CRC32C_OK : fail(HDFS_CRC32C_EHIP, "%s: %s", what, hipGetErrorString(e));
}

}  // namespace hdfs_wire

#endif  // HADOOFUS_WIRE_LAYOUT_H
