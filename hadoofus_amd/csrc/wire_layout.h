// Host side shared by libhadoofus_wire.so (wire.cpp) and
// libhadoofus_wire_batch.so (wire_batch.cpp): the layout of one write's
// stream, its packet records and the check of where a buffer lives.  One
// definition, included by both; each library keeps its own last-error text by
// defining hdfs_wire::fail itself.
#ifndef HADOOFUS_WIRE_LAYOUT_H
#define HADOOFUS_WIRE_LAYOUT_H

#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "crc32c_outpkt.h"
#include "hadoofus_crc32c.h"
#include "wire_internal.h"

namespace hdfs_wire {

// Stores the calling thread's last-error text of the including library and
// returns code.  Defined once by each library (wire.cpp, wire_batch.cpp).
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

static_assert(kChunk == hdfs_crc32c::outpkt::kWriteChunk && int64_t(kPacket) == hdfs_crc32c::outpkt::kPacketSize,
              "one packet geometry");

// Workgroups per packet, as measured (tools/wire_bench.py, DESIGN.md section
// 13): four per packet are fastest or within 4 % of the fastest from 1 MiB to
// 1 GiB.
constexpr uint32_t kSlices = 4;

struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

// ---- layout -------------------------------------------------------------------
struct Layout {
  Write w;  // pointers not set
  uint64_t nchunks = 0, wire_len = 0;
  std::vector<hdfs_crc32c::outpkt::OutPlan> plan;
};

inline bool args_ok(int proto, int ctype, int64_t offset_in_block, uint64_t len) {
  if (proto != HDFS_CRC32C_PROTO_V1 && proto != HDFS_CRC32C_PROTO_V2) return fail(HDFS_CRC32C_EINVAL, "proto must be 1 or 2"), false;
  if (ctype != HDFS_CRC32C_CSUM_NULL && ctype != HDFS_CRC32C_CSUM_CRC32 && ctype != HDFS_CRC32C_CSUM_CRC32C)
    return fail(HDFS_CRC32C_EINVAL, "bad checksum type %d", ctype), false;
  if (offset_in_block < 0) return fail(HDFS_CRC32C_EINVAL, "negative block offset"), false;
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

// ---- where the buffers live -------------------------------------------------------
// [p, p + n) inside one allocation of device `dev`.  alloc_lo / alloc_hi (may
// be NULL): that allocation's address range, for a caller that checks many
// ranges of one allocation.
inline int device_range(const void *p, uint64_t n, int dev, const char *what, uintptr_t *alloc_lo = nullptr,
                        uintptr_t *alloc_hi = nullptr) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // memory the runtime does not know: host
    return fail(HDFS_CRC32C_EINVAL, "%s: %p is not device memory", what, p);
  }
  if (a.type != hipMemoryTypeDevice) return fail(HDFS_CRC32C_EINVAL, "%s: %p is not device memory", what, p);
  if (a.device != dev)
    return fail(HDFS_CRC32C_EINVAL, "%s: memory of device %d, the engine runs on device %d", what, a.device, dev);
  void *ab = nullptr;
  size_t as = 0;
  if (hipMemGetAddressRange(&ab, &as, const_cast<void *>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(HDFS_CRC32C_EINVAL, "%s: no device allocation at %p", what, p);
  }
  const uintptr_t lo = reinterpret_cast<uintptr_t>(ab), b = reinterpret_cast<uintptr_t>(p);
  if (b < lo || b - lo > as || n > as - (b - lo))
    return fail(HDFS_CRC32C_EINVAL, "%s: %llu bytes at %p run past the end of their device allocation", what,
                (unsigned long long)n, p);
  if (alloc_lo) *alloc_lo = lo;
  if (alloc_hi) *alloc_hi = lo + as;
  return HDFS_CRC32C_OK;
}

}  // namespace hdfs_wire

#endif  // HADOOFUS_WIRE_LAYOUT_H
