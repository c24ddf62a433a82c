// libhadoofus_wirev.so: entry points of include/hadoofus_wirev.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API), the runs of whole chunks inside
// one fragment are one compute plan of that library, and both share one HIP
// runtime.  The stream's geometry and records are wire_layout.h's, the split
// of the chunk grid over the fragments and the run that computes the CRCs
// writev_layout.h's (with gather_chunks_kernel, this library's only CRC
// arithmetic); this library's own kernel (frame_gather_kernel) only moves
// bytes, with wire_frame.h's code.  It links no other companion.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "companion_support.h"
#include "crc32c_outpkt.h"
#include "hadoofus_wirev.h"
#include "wire_layout.h"
#include "wirev_internal.h"
#include "writev_layout.h"

namespace hdfs_wirev {
namespace {

using namespace hdfs_companion;
using hdfs_wire::Write;

// The store policy and the workgroups per packet are the single-write
// library's, as measured there: plain stores,
// hdfs_wire::kSlices workgroups per packet.
constexpr bool kSc1Stores = false;

// ---- the fragments ------------------------------------------------------------------
struct Frags {
  std::vector<uint64_t> lens;  // every fragment, empty ones included
  uint64_t total = 0;
  uint64_t nfrags = 0;  // the non-empty ones
};

int sum_fragments(const uint64_t *lens, const hdfs_crc32c_iovec *iov, int n, Frags &F) {
  if (n < 0) return fail(HDFS_CRC32C_EINVAL, "negative fragment count %d", n);
  if (n && !lens && !iov) return fail(HDFS_CRC32C_EINVAL, "null fragment list");
  F.lens.resize(size_t(n));
  for (int i = 0; i < n; i++) {
    const uint64_t l = lens ? lens[i] : iov[i].len;
    if (l > (uint64_t(1) << 62) - F.total) return fail(HDFS_CRC32C_EINVAL, "fragment %d: the write's length overflows", i);
    F.lens[size_t(i)] = l;
    F.total += l;
    F.nfrags += l ? 1u : 0u;
  }
  return HDFS_CRC32C_OK;
}

// Most non-empty fragments the data of one packet of plan touches.
uint32_t max_frags_per_packet(const Frags &F, const std::vector<hdfs_crc32c::outpkt::OutPlan> &plan) {
  uint32_t most = 0;
  size_t f = 0;     // the first fragment that may reach into the packet at hand
  uint64_t fa = 0;  // its offset in the write
  for (const hdfs_crc32c::outpkt::OutPlan &k : plan) {
    if (k.dlen <= 0) continue;
    const uint64_t a = k.data_off, b = a + uint64_t(k.dlen);
    while (fa + F.lens[f] <= a) fa += F.lens[f++];  // a < total: ends inside the list
    uint32_t count = 0;
    uint64_t ga = fa;
    for (size_t g = f; ga < b; g++) {
      count += F.lens[g] ? 1u : 0u;
      ga += F.lens[g];
    }
    most = std::max(most, count);
  }
  return most;
}

// ---- device scratch -----------------------------------------------------------
// The CRC array, the gather tables, the fragment table with its pinned
// staging twin and the slicing tables of one call, on the engine's device;
// grown on demand, never shrunk, kept between calls.  Calls hold g_mu from the
// table upload to the final synchronise, so one call's CRCs and tables are
// never overwritten under its kernels.
std::mutex g_mu;
struct Scratch : DeviceScratch {
  uint32_t *slice = nullptr;  // u32[2][kSliceWords]: CRC32C, CRC32 (gather_chunks_kernel's)
  DeviceBuffer crc, gtab;
  TablePair ftab;  // the fragment table

  int reserve(int to, size_t crc_bytes, size_t gtab_bytes, size_t ftab_bytes) {
    auto release_own = [this] {
      if (slice) (void)hipFree(slice);
      slice = nullptr;
      crc.release();
      gtab.release();
      ftab.release();
    };
    int rc = bind(to, "stream and tables", release_own);
    if (rc) return rc;
    if (!slice) {  // bound anew: the slicing tables
      const hipError_t e = hdfs_writev::upload_slicing_tables(&slice);
      if (e != hipSuccess) {
        unbind(release_own);
        return fail(HDFS_CRC32C_EHIP, "stream and tables: %s", hipGetErrorString(e));
      }
    }
    if ((rc = crc.reserve(crc_bytes, kScratchFloor)) || (rc = gtab.reserve(gtab_bytes, kScratchFloor))) return rc;
    return ftab.reserve(ftab_bytes, kTableFloor);
  }
} g_s;

// ---- the call -------------------------------------------------------------------------
// iters == 0: the call of hdfs_wirev_compose_packets.  iters > 0: the same,
// then the frame kernel alone iters more times between two events
// (hdfs_wirev_frame_time).
int compose(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t off, int64_t seq, int proto, int ctype, int finish,
            void *wire, uint64_t wire_cap, hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts,
            uint64_t *wire_len, void *stream, unsigned flags, int iters, double *ms_per_iter) {
  if (npkts) *npkts = 0;
  if (wire_len) *wire_len = 0;
  Frags F;
  int rc = sum_fragments(nullptr, iov, iovcnt, F);
  if (rc) return rc;
  const uint64_t len = F.total;
  if (!hdfs_wire::args_ok(proto, ctype, off, len)) return HDFS_CRC32C_EINVAL;
  hdfs_wire::Layout L;
  if ((rc = hdfs_wire::build_layout(len, off, seq, proto, ctype, finish != 0, L))) return rc;
  if (npkts) *npkts = L.plan.size();
  if (wire_len) *wire_len = L.wire_len;
  const bool fits = pkts && max_pkts >= L.plan.size();
  if (!wire) {  // size query; the records are closed-form, so they are filled when they fit
    if (fits) hdfs_wire::fill_records(L, pkts);
    return HDFS_CRC32C_OK;
  }
  for (int i = 0; i < iovcnt; i++)
    if (iov[i].len && !iov[i].base)
      return fail(HDFS_CRC32C_EINVAL, "fragment %d: null base with %llu bytes", i, (unsigned long long)iov[i].len);
  if ((pkts && !fits) || wire_cap < L.wire_len)
    return fail(HDFS_CRC32C_EINVAL, "need %zu packets / %llu stream bytes", L.plan.size(), (unsigned long long)L.wire_len);
  if (!L.wire_len) return HDFS_CRC32C_OK;  // an empty write without finish: no packet
  Write w = L.w;
  const unsigned sl = (flags >> 8) & 0xFFu;
  if (sl > hdfs_wire::kMaxSlices) return fail(HDFS_CRC32C_EINVAL, "at most %u workgroups per packet", hdfs_wire::kMaxSlices);
  if (sl) w.slices = sl;
  const bool sc1 = iters ? (flags & HDFS_WIREV_TIME_SC1) != 0 : kSc1Stores;
  if (F.nfrags >= 0xFFFFFFFFull) return fail(HDFS_CRC32C_EINVAL, "more than 2^32 - 2 fragments in one write");
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_places(iov, iovcnt, wire, L.wire_len, dev))) return rc;
  // the CRCs: the chunk grid split over the fragments (the chunk and piece limits are the gather layout's)
  const bool crcs = w.csum && len;
  hdfs_writev::Layout G;
  if (crcs) {
    std::vector<const void *> bases(static_cast<size_t>(iovcnt));
    for (int i = 0; i < iovcnt; i++) bases[size_t(i)] = iov[i].base;
    if ((rc = hdfs_writev::build_layout(F.lens.data(), bases.data(), iovcnt, off, G))) return rc;
    if (G.info.nchunks != L.nchunks || G.n0 != w.n0)
      return fail(HDFS_CRC32C_EINVAL, "internal: the gather layout and the stream's disagree about the chunk grid");
  }
  const uint32_t nf = uint32_t(F.nfrags);
  const size_t ftab_bytes = (size_t(nf) + 1) * sizeof(Frag);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, crcs ? size_t(L.nchunks) * 4 : 0, crcs ? hdfs_writev::gather_table_bytes(G) : 0,
                        ftab_bytes)) ||
      (iters && (rc = g_s.timing_events())))
    return rc;
  // the fragment table, in pinned memory: the non-empty fragments and where
  // each starts in the write, then the sentinel
  Frag *tab = g_s.ftab.pin.as<Frag>();
  uint64_t at = 0;
  uint32_t e = 0;
  for (int i = 0; i < iovcnt; i++) {
    if (!iov[i].len) continue;
    tab[e++] = Frag{static_cast<const uint8_t *>(iov[i].base), at};
    at += iov[i].len;
  }
  tab[e] = Frag{nullptr, at};
  if (e != nf || at != len) return fail(HDFS_CRC32C_EINVAL, "internal: the fragment table does not add up");
  w.data = nullptr;  // the data are the fragments'
  w.crc = g_s.crc.as<uint32_t>();
  w.wire = static_cast<uint8_t *>(wire);
  hdfs_crc32c_plan *cplan = nullptr;
  if (crcs && (rc = hdfs_writev::gather_plan(iov, G, ctype, g_s.crc.as<uint32_t>(), &cplan))) return rc;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  hipError_t he = hipMemcpyAsync(g_s.ftab.dev.p, g_s.ftab.pin.p, ftab_bytes, hipMemcpyHostToDevice, st);
  if (he == hipSuccess && crcs)
    rc = hdfs_writev::enqueue_gather(G, cplan, ctype, g_s.gtab.p, g_s.slice, g_s.crc.as<uint32_t>(), st, &he);
  // the CRC array and the tables are out of use when either returns, so before the lock goes
  if (rc || he != hipSuccess) return sync_and_report(st, he, rc, cplan, "gather wire stream");
  rc = hdfs_wire::timed_frame_run(st, hipSuccess, nullptr, g_s.ev, iters, ms_per_iter, "gather wire stream",
                                  [&] { return launch_frame_gather(w, g_s.ftab.dev.as<Frag>(), nf, sc1, st); });
  if (cplan) hdfs_crc32c_plan_destroy(cplan);
  if (rc) return rc;
  if (fits) hdfs_wire::fill_records(L, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wirev

using namespace hdfs_wirev;

extern "C" {

int hdfs_wirev_abi_version(void) { return HDFS_WIREV_ABI_VERSION; }

const char *hdfs_wirev_last_error(void) { return last_error(); }

int hdfs_wirev_layout(const uint64_t *lens, int iovcnt, int64_t offset_in_block, int proto, int ctype, int finish,
                      hdfs_wirev_layout_info *out) {
  if (!out) return fail(HDFS_CRC32C_EINVAL, "null out");
  if (iovcnt > 0 && !lens) return fail(HDFS_CRC32C_EINVAL, "null fragment list");
  Frags F;
  int rc = sum_fragments(lens, nullptr, iovcnt, F);
  if (rc) return rc;
  if (!hdfs_wire::args_ok(proto, ctype, offset_in_block, F.total)) return HDFS_CRC32C_EINVAL;
  hdfs_wire::Layout L;
  if ((rc = hdfs_wire::build_layout(F.total, offset_in_block, 0, proto, ctype, finish != 0, L))) return rc;
  hdfs_writev::Layout G;
  if ((rc = hdfs_writev::build_layout(F.lens.data(), nullptr, iovcnt, offset_in_block, G))) return rc;
  std::memset(out, 0, sizeof(*out));
  out->npkts = L.plan.size();
  out->nchunks = L.nchunks;
  out->wire_len = L.wire_len;
  out->packet_stride = L.w.hb + (L.w.csum ? 4u * (hdfs_wire::kPacket / hdfs_wire::kChunk) : 0u) + hdfs_wire::kPacket;
  out->header_bytes = L.w.hb;
  out->head_bytes = L.w.n0;
  out->nsegments = G.info.nsegments;
  out->seg_chunks = G.info.seg_chunks;
  out->ngathered = G.info.ngathered;
  out->npieces = G.info.npieces;
  out->max_pieces = G.info.max_pieces;
  out->nfrags = F.nfrags;
  out->max_frags_per_packet = max_frags_per_packet(F, L.plan);
  return HDFS_CRC32C_OK;
}

int hdfs_wirev_compose_packets(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int64_t seqno,
                               int proto, int ctype, int finish, void *wire, uint64_t wire_cap,
                               hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, uint64_t *wire_len,
                               void *stream) {
  return compose(iov, iovcnt, offset_in_block, seqno, proto, ctype, finish, wire, wire_cap, pkts, max_pkts, npkts,
                 wire_len, stream, 0u, 0, nullptr);
}

int hdfs_wirev_frame_time(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int proto, int ctype,
                          int finish, void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter) {
  if (iters < 1 || !ms_per_iter || !wire) return fail(HDFS_CRC32C_EINVAL, "iters >= 1, a stream buffer and ms_per_iter are needed");
  return compose(iov, iovcnt, offset_in_block, 0, proto, ctype, finish, wire, wire_cap, nullptr, 0, nullptr, nullptr,
                 nullptr, flags, iters, ms_per_iter);
}

}  // extern "C"
