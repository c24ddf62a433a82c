// libhadoofus_wirev_fused.so: entry points of include/hadoofus_wirev_fused.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Unlike libhadoofus_wirev.so it asks that library for no CRC and has no
// gather layout: its own kernel (frame_fused_gather_kernel) computes the chunk
// CRCs from the bytes it copies out of the fragments, from tables
// (wire_fused_host.h) built out of crc32c_tables.h, and finds the fragments through one table uploaded
// per call.  The stream's geometry and records are wire_layout.h's.  It links
// no other companion.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "companion_support.h"
#include "crc32c_outpkt.h"
#include "hadoofus_wirev_fused.h"
#include "wire_fused_host.h"
#include "wire_fused_tables.h"
#include "wire_layout.h"
#include "wirev_fused_internal.h"
#include "wirev_fused_lookup.h"

namespace hdfs_wirev_fused {
namespace {

using namespace hdfs_companion;

// ---- the fragments ------------------------------------------------------------------
// Where every non-empty fragment starts in the write, and the write's length
// behind them: the `at` column of the kernel's table.
struct Frags {
  std::vector<uint64_t> at;
  uint64_t total = 0;
  uint64_t nfrags() const { return at.size() - 1; }
};

int sum_fragments(const uint64_t *lens, const hdfs_crc32c_iovec *iov, int n, Frags &F) {
  if (n < 0) return fail(HDFS_CRC32C_EINVAL, "negative fragment count %d", n);
  if (n && !lens && !iov) return fail(HDFS_CRC32C_EINVAL, "null fragment list");
  F.at.reserve(size_t(n) + 1);
  for (int i = 0; i < n; i++) {
    const uint64_t l = lens ? lens[i] : iov[i].len;
    if (l > (uint64_t(1) << 62) - F.total) return fail(HDFS_CRC32C_EINVAL, "fragment %d: the write's length overflows", i);
    if (l) F.at.push_back(F.total);
    F.total += l;
  }
  F.at.push_back(F.total);
  return HDFS_CRC32C_OK;
}

// ---- device state -------------------------------------------------------------
// The CRC tables on the engine's device and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept;
// the fragment table with its pinned staging twin, grown on demand, never
// shrunk, kept between calls.  Calls
// hold g_mu from the table's upload to the final synchronise, so one call's
// table is never overwritten under its kernel.
std::mutex g_mu;
using Fused = hdfs_wire_fused::DeviceState<prepare_frame_fused_gather, kMaxGroups>;
struct Scratch : DeviceScratch {
  Fused fused;
  TablePair ftab;  // the fragment table

  int reserve(int to, size_t ftab_bytes) {
    int rc = bind(to, "stream and tables", [this] {
      fused.release();
      ftab.release();
    });
    if (rc || (rc = fused.setup(to))) return rc;
    return ftab.reserve(ftab_bytes, kTableFloor);
  }
} g_s;

// ---- the call -------------------------------------------------------------------------
// iters == 0: the call of hdfs_wirev_fused_compose_packets.  iters > 0: the
// same, then the kernel alone iters more times between two events
// (hdfs_wirev_fused_time).
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
  if ((rc = Fused::flags_ok(flags))) return rc;
  if (F.nfrags() >= 0xFFFFFFFFull) return fail(HDFS_CRC32C_EINVAL, "more than 2^32 - 2 fragments in one write");
  if (!L.wire_len) return HDFS_CRC32C_OK;  // an empty write without finish: no packet
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_places(iov, iovcnt, wire, L.wire_len, dev))) return rc;
  const uint32_t nf = uint32_t(F.nfrags());
  const size_t ftab_bytes = (size_t(nf) + 1) * sizeof(Frag);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, ftab_bytes)) || (iters && (rc = g_s.timing_events()))) return rc;
  // the fragment table, in pinned memory: the non-empty fragments and where
  // each starts in the write, then the sentinel
  Frag *ft = g_s.ftab.pin.as<Frag>();
  uint32_t e = 0;
  for (int i = 0; i < iovcnt; i++)
    if (iov[i].len) {
      ft[e] = Frag{static_cast<const uint8_t *>(iov[i].base), F.at[e]};
      e++;
    }
  ft[e] = Frag{nullptr, len};
  if (e != nf) return fail(HDFS_CRC32C_EINVAL, "internal: the fragment table does not add up");
  hdfs_wire::Write w = L.w;
  w.data = nullptr;  // the data are the fragments': the kernel counts in their concatenation
  w.crc = nullptr;
  w.wire = static_cast<uint8_t *>(wire);
  const uint32_t *tab = g_s.fused.tables(ctype);
  const uint32_t groups = g_s.fused.grid(flags, w.npk);
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  const hipError_t he = hipMemcpyAsync(g_s.ftab.dev.p, g_s.ftab.pin.p, ftab_bytes, hipMemcpyHostToDevice, st);
  // the table is out of use when this returns, so before the lock goes
  rc = hdfs_wire::timed_frame_run(st, he, nullptr, g_s.ev, iters, ms_per_iter, "fused gather wire stream",
                                  [&] { return launch_frame_fused_gather(w, g_s.ftab.dev.as<Frag>(), nf, tab, groups, st); });
  if (rc) return rc;
  if (fits) hdfs_wire::fill_records(L, pkts);
  return HDFS_CRC32C_OK;
}

}  // namespace
}  // namespace hdfs_wirev_fused

using namespace hdfs_wirev_fused;

extern "C" {

int hdfs_wirev_fused_abi_version(void) { return HDFS_WIREV_FUSED_ABI_VERSION; }

const char *hdfs_wirev_fused_last_error(void) { return last_error(); }

int hdfs_wirev_fused_layout(const uint64_t *lens, int iovcnt, int64_t offset_in_block, int proto, int ctype,
                            int finish, hdfs_wirev_fused_layout_info *out) {
  if (!out) return fail(HDFS_CRC32C_EINVAL, "null out");
  if (iovcnt > 0 && !lens) return fail(HDFS_CRC32C_EINVAL, "null fragment list");
  Frags F;
  int rc = sum_fragments(lens, nullptr, iovcnt, F);
  if (rc) return rc;
  if (!hdfs_wire::args_ok(proto, ctype, offset_in_block, F.total)) return HDFS_CRC32C_EINVAL;
  if (F.nfrags() >= 0xFFFFFFFFull) return fail(HDFS_CRC32C_EINVAL, "more than 2^32 - 2 fragments in one write");
  hdfs_wire::Layout L;
  if ((rc = hdfs_wire::build_layout(F.total, offset_in_block, 0, proto, ctype, finish != 0, L))) return rc;
  RoundCounts c;
  uint32_t hint = 0;
  for (const hdfs_crc32c::outpkt::OutPlan &k : L.plan)
    if (k.dlen > 0) count_packet(F.at.data(), uint32_t(F.nfrags()), k.data_off, uint32_t(k.dlen), hint, c);
  std::memset(out, 0, sizeof(*out));
  out->npkts = L.plan.size();
  out->nchunks = L.nchunks;
  out->wire_len = L.wire_len;
  out->nfrags = F.nfrags();
  out->rounds = c.rounds;
  out->seamed_rounds = c.seamed_rounds;
  out->seamed_ragged = c.seamed_ragged;
  out->packet_stride = L.w.hb + (L.w.csum ? 4u * (hdfs_wire::kPacket / hdfs_wire::kChunk) : 0u) + hdfs_wire::kPacket;
  out->header_bytes = L.w.hb;
  out->head_bytes = L.w.n0;
  out->max_frags_per_round = c.max_frags_per_round;
  return HDFS_CRC32C_OK;
}

int hdfs_wirev_fused_compose_packets(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int64_t seqno,
                                     int proto, int ctype, int finish, void *wire, uint64_t wire_cap,
                                     hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, uint64_t *wire_len,
                                     void *stream) {
  return compose(iov, iovcnt, offset_in_block, seqno, proto, ctype, finish, wire, wire_cap, pkts, max_pkts, npkts,
                 wire_len, stream, 0u, 0, nullptr);
}

int hdfs_wirev_fused_time(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int proto, int ctype,
                          int finish, void *wire, uint64_t wire_cap, unsigned flags, int iters, double *ms_per_iter) {
  if (iters < 1 || !ms_per_iter || !wire)
    return fail(HDFS_CRC32C_EINVAL, "iters >= 1, a stream buffer and ms_per_iter are needed");
  return compose(iov, iovcnt, offset_in_block, 0, proto, ctype, finish, wire, wire_cap, nullptr, 0, nullptr, nullptr,
                 nullptr, flags, iters, ms_per_iter);
}

}  // extern "C"
