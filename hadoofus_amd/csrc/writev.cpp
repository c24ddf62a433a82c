// libhadoofus_writev.so: entry points of include/hadoofus_writev.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API), the bulk of a gather write runs
// as one compute plan of that library, and both share one HIP runtime.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "companion_support.h"
#include "crc32c_outpkt.h"
#include "hadoofus_writev.h"
#include "writev_internal.h"
#include "writev_layout.h"

namespace hdfs_writev {
namespace {

using namespace hdfs_companion;
using namespace hdfs_crc32c::outpkt;

constexpr uint64_t kHostWindow = uint64_t(64) << 20;  // host fragments: bytes packed per call of the main library

// The layout of a gather write (Run, Layout, build_layout, kMinSegChunks), the
// slicing tables and the run that leaves the chunk CRCs in a device array
// (gather_plan, enqueue_gather) are writev_layout.h's, shared with the
// gather-wire library.

// ---- device scratch -----------------------------------------------------------
// The CRC array, the chunk and piece tables and the pinned landing area of one
// call, on the engine's device; grown on demand, never shrunk, kept between
// calls.  Calls hold g_mu from the uploads to the final synchronise, so one
// call's tables are never overwritten under its kernels.
std::mutex g_mu;
// The pinned landing area is the engine's pin registry's, not the runtime's.
int landing_alloc(void **p, size_t n) {
  const int rc = hdfs_crc32c_host_alloc(p, n);
  return rc ? engine_fail(rc, "pinned CRC landing area") : rc;
}
void landing_free(void *p) { (void)hdfs_crc32c_host_free(p); }

struct Scratch : DeviceScratch {
  uint32_t *slice = nullptr;  // u32[2][kSliceWords]: CRC32C, CRC32
  DeviceBuffer crc, tab;
  PinnedBuffer<landing_alloc, landing_free> h_crc;

  int reserve(int to, size_t crc_bytes, size_t tab_bytes) {
    auto release_own = [this] {
      if (slice) (void)hipFree(slice);
      slice = nullptr;
      crc.release();
      tab.release();
      h_crc.release();
    };
    int rc = bind(to, "stream and tables", release_own);
    if (rc) return rc;
    if (!slice) {  // bound anew: the slicing tables
      const hipError_t e = upload_slicing_tables(&slice);
      if (e != hipSuccess) {
        unbind(release_own);
        return fail(HDFS_CRC32C_EHIP, "stream and tables: %s", hipGetErrorString(e));
      }
    }
    if ((rc = crc.reserve(crc_bytes, kScratchFloor)) || (rc = tab.reserve(tab_bytes, kScratchFloor))) return rc;
    return h_crc.reserve(crc_bytes, kScratchFloor);
  }
} g_s;

// ---- where the fragments live ---------------------------------------------------
// All device memory of device `dev` (each inside one allocation) or all host
// memory; zero-length fragments say nothing.
int classify(const hdfs_crc32c_iovec *iov, int n, int dev, bool *on_device) {
  uintptr_t lo = 0, hi = 0;  // the device allocation the last query found
  int first = -1;
  bool first_dev = false;
  for (int i = 0; i < n; i++) {
    if (!iov[i].len) continue;
    const uintptr_t b = reinterpret_cast<uintptr_t>(iov[i].base);
    bool d = b >= lo && b < hi;
    if (!d) {
      const Placement w = placement(iov[i].base, dev);
      if (w.kind == Placement::kDevice) {  // memory the runtime does not know is host memory
        if (w.device != dev)
          return fail(HDFS_CRC32C_EINVAL, "fragment %d: memory of device %d, the engine runs on device %d", i, w.device, dev);
        if (!w.hi) return fail(HDFS_CRC32C_EINVAL, "fragment %d: no device allocation at %p", i, iov[i].base);
        lo = w.lo;
        hi = w.hi;
        d = true;
      }
    }
    if (d && iov[i].len > hi - b)
      return fail(HDFS_CRC32C_EINVAL, "fragment %d: %llu bytes at %p run past the end of its device allocation", i,
                  (unsigned long long)iov[i].len, iov[i].base);
    if (first < 0) {
      first = i;
      first_dev = d;
    } else if (d != first_dev) {
      return fail(HDFS_CRC32C_EINVAL, "fragment %d is %s memory, fragment %d is %s memory: mixed fragments", i,
                  d ? "device" : "host", first, first_dev ? "device" : "host");
    }
  }
  *on_device = first_dev;
  return HDFS_CRC32C_OK;
}

// ---- device fragments -------------------------------------------------------------
int compose_device(const hdfs_crc32c_iovec *iov, const Layout &L, int dev, const std::vector<OutPlan> &plan,
                   int proto, int ctype, uint8_t *hdr_out, hdfs_crc32c_out_packet *pkts) {
  const hdfs_writev_layout_info &I = L.info;
  const size_t crc_bytes = size_t(I.nchunks) * 4;
  DeviceGuard g(dev);
  std::lock_guard<std::mutex> lk(g_mu);
  int rc = g_s.reserve(dev, crc_bytes, gather_table_bytes(L));
  if (rc) return rc;
  uint32_t *d_crc = g_s.crc.as<uint32_t>();
  hdfs_crc32c_plan *cplan = nullptr;
  if ((rc = gather_plan(iov, L, ctype, d_crc, &cplan))) return rc;
  hipStream_t st = g_s.st;
  hipError_t e = hipSuccess;
  rc = enqueue_gather(L, cplan, ctype, g_s.tab.p, g_s.slice, d_crc, st, &e);
  if (e == hipSuccess && !rc) e = hipMemcpyAsync(g_s.h_crc.p, d_crc, crc_bytes, hipMemcpyDeviceToHost, st);
  // always: the tables and the CRC array must be out of use before the lock goes
  if ((rc = sync_and_report(st, e, rc, cplan, "gather write"))) return rc;
  const uint32_t *crcs = g_s.h_crc.as<const uint32_t>();
  write_out_packets(plan, proto, true, L.n0, crcs, crcs + (L.n0 ? 1 : 0), hdr_out, pkts);
  return HDFS_CRC32C_OK;
}

// ---- host fragments ------------------------------------------------------------------
// Packed window by window (whole packets of the write's plan, at most
// kHostWindow bytes) into one host buffer; hdfs_crc32c_compose_packets does
// each window at its running block offset and sequence number.
int compose_host(const hdfs_crc32c_iovec *iov, uint64_t total, int64_t off, int64_t seq, int proto, int ctype,
                 bool finish, uint8_t *hdr_out, uint64_t hdr_cap, hdfs_crc32c_out_packet *pkts, size_t max_pkts) {
  std::vector<OutPlan> plan;
  plan_out_packets(total, off, seq, false, plan);
  std::unique_ptr<uint8_t[]> win(new uint8_t[size_t(std::min(total, kHostWindow))]);
  int f = 0;        // fragment cursor
  uint64_t fo = 0;  // bytes of fragment f already packed
  uint64_t hpos = 0;
  size_t np = 0;
  for (size_t i = 0; i < plan.size();) {
    size_t j = i;
    uint64_t wlen = 0;
    while (j < plan.size() && wlen + uint64_t(plan[j].dlen) <= kHostWindow) wlen += uint64_t(plan[j++].dlen);
    for (uint64_t got = 0; got < wlen;) {
      const uint64_t take = std::min(wlen - got, iov[f].len - fo);
      if (take) std::memcpy(win.get() + got, static_cast<const uint8_t *>(iov[f].base) + fo, size_t(take));
      got += take;
      fo += take;
      if (fo == iov[f].len && got < wlen) {
        f++;
        fo = 0;
      }
    }
    size_t wn = 0;
    uint64_t wused = 0;
    const int rc = hdfs_crc32c_compose_packets(win.get(), wlen, plan[i].offset, plan[i].seqno, proto, ctype,
                                               finish && j == plan.size() ? 1 : 0, hdr_out + hpos, hdr_cap - hpos,
                                               pkts + np, max_pkts - np, &wn, &wused);
    if (rc) return engine_fail(rc, "compose_packets");
    for (size_t k = np; k < np + wn; k++) {
      pkts[k].hdr_off += hpos;
      pkts[k].data_off += plan[i].data_off;
    }
    np += wn;
    hpos += wused;
    i = j;
  }
  return HDFS_CRC32C_OK;
}

bool args_ok(int proto, int ctype, int64_t offset_in_block) { return packet_args_ok(proto, ctype, offset_in_block); }

}  // namespace
}  // namespace hdfs_writev

using namespace hdfs_writev;

extern "C" {

int hdfs_writev_abi_version(void) { return HDFS_WRITEV_ABI_VERSION; }

const char *hdfs_writev_last_error(void) { return last_error(); }

int hdfs_writev_layout(const uint64_t *lens, int iovcnt, int64_t offset_in_block, hdfs_writev_layout_info *out) {
  if (!out) return fail(HDFS_CRC32C_EINVAL, "null out");
  if (iovcnt < 0 || (iovcnt && !lens)) return fail(HDFS_CRC32C_EINVAL, "null or negative fragment list");
  if (offset_in_block < 0) return fail(HDFS_CRC32C_EINVAL, "negative block offset");
  Layout L;
  const int rc = build_layout(lens, nullptr, iovcnt, offset_in_block, L);
  if (rc) return rc;
  *out = L.info;
  return HDFS_CRC32C_OK;
}

int hdfs_writev_compose_packets(const hdfs_crc32c_iovec *iov, int iovcnt, int64_t offset_in_block, int64_t seqno,
                                int proto, int ctype, int finish, void *hdr_out, uint64_t hdr_cap,
                                hdfs_crc32c_out_packet *pkts, size_t max_pkts, size_t *npkts, uint64_t *hdr_used) {
  if (npkts) *npkts = 0;
  if (hdr_used) *hdr_used = 0;
  if (iovcnt < 0) return fail(HDFS_CRC32C_EINVAL, "negative fragment count %d", iovcnt);
  if (iovcnt && !iov) return fail(HDFS_CRC32C_EINVAL, "null fragment list");
  if (!args_ok(proto, ctype, offset_in_block)) return HDFS_CRC32C_EINVAL;
  uint64_t total = 0;
  for (int i = 0; i < iovcnt; i++) {
    if (iov[i].len && !iov[i].base) return fail(HDFS_CRC32C_EINVAL, "fragment %d: null base with %llu bytes", i,
                                                (unsigned long long)iov[i].len);
    if (iov[i].len > (uint64_t(1) << 62) - total) return fail(HDFS_CRC32C_EINVAL, "fragment %d: the write's length overflows", i);
    total += iov[i].len;
  }
  int rc;
  const bool csum = ctype != HDFS_CRC32C_CSUM_NULL;
  std::vector<OutPlan> plan;
  plan_out_packets(total, offset_in_block, seqno, finish != 0, plan);
  const uint64_t need = out_plan_bytes(plan, proto, csum);
  if (npkts) *npkts = plan.size();
  if (hdr_used) *hdr_used = need;
  if (!hdr_out || !pkts) return HDFS_CRC32C_OK;  // size query
  if (max_pkts < plan.size() || hdr_cap < need)
    return fail(HDFS_CRC32C_EINVAL, "need %zu packets / %llu header bytes", plan.size(), (unsigned long long)need);
  uint8_t *out = static_cast<uint8_t *>(hdr_out);
  if (!csum || !total) {  // sizing and headers only
    write_out_packets(plan, proto, false, 0, nullptr, nullptr, out, pkts);
    return HDFS_CRC32C_OK;
  }
  if (iovcnt == 1) {
    rc = hdfs_crc32c_compose_packets(iov[0].base, iov[0].len, offset_in_block, seqno, proto, ctype, finish, hdr_out,
                                     hdr_cap, pkts, max_pkts, npkts, hdr_used);
    return rc ? engine_fail(rc, "compose_packets") : rc;
  }
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  bool on_device = false;
  {
    DeviceGuard g(dev);
    if ((rc = classify(iov, iovcnt, dev, &on_device))) return rc;
  }
  if (!on_device)
    return compose_host(iov, total, offset_in_block, seqno, proto, ctype, finish != 0, out, hdr_cap, pkts, max_pkts);
  std::vector<uint64_t> lens(static_cast<size_t>(iovcnt));
  std::vector<const void *> bases(static_cast<size_t>(iovcnt));
  for (int i = 0; i < iovcnt; i++) {
    lens[i] = iov[i].len;
    bases[i] = iov[i].base;
  }
  Layout L;
  if ((rc = build_layout(lens.data(), bases.data(), iovcnt, offset_in_block, L))) return rc;
  return compose_device(iov, L, dev, plan, proto, ctype, out, pkts);
}

}  // extern "C"
