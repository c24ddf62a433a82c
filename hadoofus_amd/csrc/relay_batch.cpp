// libhadoofus_relay_batch.so: entry points of include/hadoofus_relay_batch.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API) and both share one HIP runtime.
// Its kernels (relay_batch_kernels.hip) verify the regular entries of a batch
// and re-frame them as writes in one pass; the CRC tables are the fused write
// libraries' (wire_fused_host.h, built out of crc32c_tables.h).  Every other
// entry is served here after the synchronise: hdfs_crc32c_read_packets into
// the library's scratch buffer, then the fused batch write library's kernel
// (wire_fused_batch_kernels.hip, compiled into this library as it stands) over
// a table of that one write, laid out by wire_layout.h.  This file holds no
// walk and no framing of its own.  The run, the collection of the entries'
// outcomes and the base of the scratch are read_batch_host.h's, the overlap
// sweep companion_support.h's.
#include <hip/hip_runtime.h>

#include <mutex>
#include <vector>

#include "companion_support.h"
#include "hadoofus_relay_batch.h"
#include "read_batch_host.h"
#include "read_batch_layout.h"
#include "relay_batch_internal.h"
#include "relay_batch_lookup.h"
#include "wire_fused_batch_internal.h"
#include "wire_fused_host.h"
#include "wire_fused_tables.h"
#include "wire_layout.h"

namespace hdfs_relay_batch {
namespace {

using namespace hdfs_companion;
using hdfs_wire::Layout;
using hdfs_wire::Write;

static_assert(HDFS_RELAY_BATCH_MAX_ENTRIES == kMaxEntries, "the header's limit is the probe's");

// Both kernels keep the table image in LDS: each is allowed its size once per device.
hipError_t prepare_both() {
  const hipError_t e = prepare_relay_fused_batch();
  return e == hipSuccess ? hdfs_wire_fused::prepare_frame_fused_batch() : e;
}

// ---- device state -------------------------------------------------------------
// On the engine's device: the CRC tables and the workgroups of one launch
// (wire_fused_host.h), set up when the library is first used there and kept;
// the call's device tables and their pinned twin, the one-write table of a
// fallback entry with its twin, and the fallback's payload buffer, all grown on
// demand, never shrunk, kept between calls.  Calls hold g_mu from the tables'
// upload to the last fallback entry.
std::mutex g_mu;
using Fused = hdfs_wire_fused::DeviceState<prepare_both, kBatchMaxGroups>;
struct Scratch : ReadScratch<Fused> {
  TablePair one;
  DeviceBuffer payload;

  int reserve(int to, size_t tab_bytes) {
    return ReadScratch::reserve(to, tab_bytes, [this] {
      one.release();
      payload.release();
    });
  }
} g_s;

void clear_outputs(hdfs_relay_batch_entry *e, size_t n) {
  for (size_t b = 0; b < n; b++) {
    e[b].consumed = e[b].delivered = e[b].wire_len = e[b].npkts = 0;
    e[b].src_offset_in_block = 0;
    e[b].rc = 0;
    e[b].path = HDFS_RELAY_BATCH_PATH_FALLBACK;
  }
}

// ---- argument checks that need no device ------------------------------------------
int check_arguments(hdfs_relay_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype) {
  if (!e || !n) return fail(HDFS_CRC32C_EINVAL, "no entries");
  if (n > kMaxEntries)
    return fail(HDFS_CRC32C_EINVAL, "%zu entries, at most %u in one call", n, unsigned(kMaxEntries));
  clear_outputs(e, n);
  if (!packet_args_ok(proto, ctype, 0)) return prefix_fail(HDFS_CRC32C_EINVAL, "entry 0");
  if (ctype == HDFS_CRC32C_CSUM_NULL)
    return fail(HDFS_CRC32C_EINVAL, "entry 0: verify + re-frame needs CRC32 or CRC32C");
  if (!chunk_size) return fail(HDFS_CRC32C_EINVAL, "entry 0: chunk_size 0");
  for (size_t b = 0; b < n; b++) {
    if (e[b].len && !e[b].stream) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null stream", b);
    if (e[b].wire_cap && !e[b].wire) return fail(HDFS_CRC32C_EINVAL, "entry %zu: null wire", b);
    if (!packet_args_ok(proto, ctype, e[b].offset_in_block)) return prefix_fail(HDFS_CRC32C_EINVAL, "entry %zu", b);
    if (e[b].seqno < 0) return fail(HDFS_CRC32C_EINVAL, "entry %zu: negative seqno", b);
  }
  return HDFS_CRC32C_OK;
}

// ---- where the buffers lie -----------------------------------------------------------
// Every range inside one allocation of device `dev`; no wire range overlaps a
// stream or another wire range.  An entry with len == 0 names no stream range,
// one with wire_cap == 0 no wire range.
int check_batch_places(const hdfs_relay_batch_entry *e, size_t n, int dev) {
  int rc;
  Allocations al;
  std::vector<Span> wires, streams;
  wires.reserve(n);
  streams.reserve(n);
  for (size_t b = 0; b < n; b++) {
    if ((e[b].len && (rc = al.check(e[b].stream, e[b].len, dev, "stream"))) ||
        (e[b].wire_cap && (rc = al.check(e[b].wire, e[b].wire_cap, dev, "wire"))))
      return prefix_fail(rc, "entry %zu", b);
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(e[b].stream), w0 = reinterpret_cast<uintptr_t>(e[b].wire);
    if (e[b].len) streams.push_back(Span{s0, s0 + uintptr_t(e[b].len), uint32_t(b), 0u});
    if (e[b].wire_cap) wires.push_back(Span{w0, w0 + uintptr_t(e[b].wire_cap), uint32_t(b), 1u});
  }
  return check_overlaps(wires, streams, nullptr, nullptr, SpanNouns{"wire", "stream"});
}

// ---- the layout of a write ---------------------------------------------------------------
// wire_layout.h's, which checks every packet against outpkt::plan_out_packets;
// for a write on the chunk grid the closed form the probe uses must say the same.
int layout_write(uint64_t payload, int64_t off, int64_t seq, int proto, int ctype, bool finish, Layout &L) {
  if (!hdfs_wire::args_ok(proto, ctype, off, payload)) return HDFS_CRC32C_EINVAL;
  const int rc = hdfs_wire::build_layout(payload, off, seq, proto, ctype, finish, L);
  if (rc) return rc;
  if (ctype != HDFS_CRC32C_CSUM_NULL && uint64_t(off) % kGrid == 0u) {
    uint64_t wire_len = 0, npk = 0;
    out_shape(payload, L.w.hb, finish, wire_len, npk);
    if (wire_len != L.wire_len || npk != L.plan.size())
      return fail(HDFS_CRC32C_EINVAL, "internal: the closed form of an aligned write's stream is not its plan");
  }
  return HDFS_CRC32C_OK;
}

// ---- an entry served after the synchronise --------------------------------------------------
// The read: exactly the call of the contract, into the library's buffer (the
// payload is shorter than the stream), the walk not cut (read_unlimited).
// Then, where the read is clean and the stream
// fits, the write: frame_fused_batch_kernel over a table of this one write.
int fallback(hdfs_relay_batch_entry &x, size_t b, int proto, uint32_t chunk_size, int ctype, hipStream_t st) {
  x.path = HDFS_RELAY_BATCH_PATH_FALLBACK;
  int rc = g_s.payload.reserve(size_t(x.len), kScratchFloor);
  if (rc) return x.rc = rc, prefix_fail(rc, "entry %zu", b);
  const hdfs_crc32c_iovec iov{g_s.payload.p, x.len};
  size_t np = 0;
  uint64_t used = 0, got = 0;
  rc = read_unlimited(g_s.recs, x.stream, x.len, proto, chunk_size, ctype, 0, HDFS_CRC32C_READ_ALL, &iov, 1, nullptr, 0,
                      &np, &used, &got);
  x.rc = rc;
  if (rc < 0) return engine_fail(rc, "read_packets"), prefix_fail(rc, "entry %zu", b);
  x.consumed = used;
  x.delivered = got;
  x.src_offset_in_block = np ? g_s.recs[0].offset_in_block : 0;
  if (rc) return rc;  // the read found an error: no stream
  Layout L;
  if ((rc = layout_write(got, x.offset_in_block, x.seqno, proto, ctype, x.finish != 0, L)))
    return x.rc = rc, prefix_fail(rc, "entry %zu", b);
  if (L.wire_len > x.wire_cap) {
    x.rc = HDFS_CRC32C_EINVAL;
    return fail(HDFS_CRC32C_EINVAL, "entry %zu: the write's stream of %llu bytes does not fit wire_cap %llu", b,
                (unsigned long long)L.wire_len, (unsigned long long)x.wire_cap);
  }
  if (!L.plan.empty()) {
    const uint32_t npk = uint32_t(L.plan.size());
    const size_t bytes = hdfs_wire_fused::fused_batch_table_bytes(1);
    if ((rc = g_s.one.reserve(bytes, kTableFloor))) return x.rc = rc, prefix_fail(rc, "entry %zu", b);
    Write *t = g_s.one.pin.as<Write>();
    *t = L.w;
    t->data = g_s.payload.as<uint8_t>();
    t->crc = nullptr;
    t->wire = static_cast<uint8_t *>(x.wire);
    uint32_t *pk0 = reinterpret_cast<uint32_t *>(t + 1);
    pk0[0] = 0u;
    pk0[1] = npk;
    hipError_t he = hipMemcpyAsync(g_s.one.dev.p, g_s.one.pin.p, bytes, hipMemcpyHostToDevice, st);
    if (he == hipSuccess)
      he = hdfs_wire_fused::launch_frame_fused_batch(g_s.one.dev.p, 1u, npk, uint32_t(proto), true,
                                                     g_s.fused.tables(ctype), g_s.fused.grid(0u, npk), st);
    if ((rc = sync_and_report(st, he, HDFS_CRC32C_OK, nullptr, "relay batch"))) return x.rc = rc, prefix_fail(rc, "entry %zu", b);
  }
  x.wire_len = L.wire_len;
  x.npkts = L.plan.size();
  return HDFS_CRC32C_OK;
}

// ---- the call -------------------------------------------------------------------------
// timing == false: the call of hdfs_relay_batch_relay.  timing: the same on the
// library's stream, then both launches alone iters more times between two
// events (hdfs_relay_batch_time).
int relay(hdfs_relay_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype, void *stream, bool timing,
          unsigned flags, int iters, double *ms_per_iter) {
  if (ms_per_iter) *ms_per_iter = 0;
  int rc = check_arguments(e, n, proto, chunk_size, ctype);
  if (rc) return rc;
  if (timing) {  // decided by the arguments alone, before any device is asked
    if ((rc = timing_args_ok(iters, ms_per_iter)) || (rc = Fused::flags_ok(flags))) return rc;
  }
  int dev = -1;
  if ((rc = engine_device(&dev))) return rc;
  DeviceGuard g(dev);
  if ((rc = check_batch_places(e, n, dev))) return rc;
  const Tables T(n);
  const uint32_t hb = hdfs_crc32c::outpkt::out_header_bytes(proto);
  std::lock_guard<std::mutex> lk(g_mu);
  if ((rc = g_s.reserve(dev, T.bytes)) || (timing && (rc = g_s.timing_events()))) return rc;
  // the entries, in pinned memory; one without a stream is uploaded empty, so the probe gives it no slot
  uint8_t *pin = g_s.tab.pin.as<uint8_t>(), *dv = g_s.tab.dev.as<uint8_t>();
  Entry *in = reinterpret_cast<Entry *>(pin + T.in);
  for (size_t b = 0; b < n; b++)
    in[b] = Entry{e[b].len ? static_cast<const uint8_t *>(e[b].stream) : nullptr,
                  e[b].len,
                  static_cast<uint8_t *>(e[b].wire),
                  e[b].wire_cap,
                  e[b].offset_in_block,
                  e[b].seqno,
                  e[b].finish ? 1u : 0u,
                  hb};
  const uint32_t *crc_tab = g_s.fused.tables(ctype);
  const uint32_t groups = (flags >> 8) ? (flags >> 8) : g_s.fused.groups;
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : g_s.st;
  auto launches = [&] {
    hipError_t le = launch_probe(dv, uint32_t(n), proto, chunk_size, ctype, st);
    if (le == hipSuccess) le = launch_relay_fused_batch(dv, uint32_t(n), uint32_t(proto), crc_tab, groups, st);
    return le;
  };
  if ((rc = probed_run(st, g_s.tab, T.in, n * sizeof(Entry), T.desc, T.bytes, g_s.ev, timing ? iters : 0, ms_per_iter,
                       "relay batch", launches)))
    return rc;
  const Desc *desc = reinterpret_cast<const Desc *>(pin + T.desc);
  const uint32_t *slot = reinterpret_cast<const uint32_t *>(pin + T.slot);
  const uint32_t *status = reinterpret_cast<const uint32_t *>(pin + T.status);
  const uint32_t nreg = reinterpret_cast<const uint32_t *>(pin + T.meta)[0];
  Outcomes out;
  for (size_t b = 0; b < n; b++) {
    hdfs_relay_batch_entry &x = e[b];
    const uint32_t s = slot[b];
    if (!slot_adds_up(s, kNoSlot, nreg, b, [&](uint32_t i) { return desc[i].in.entry; }) ||
        (s != kNoSlot && (in_packets(desc[s].g) != desc[s].in.npk || desc[s].wire_len > x.wire_cap)))
      return tables_fail(b);
    if (s != kNoSlot && !status[s]) {
      const Desc &d = desc[s];
      x.rc = 0;
      x.path = HDFS_RELAY_BATCH_PATH_KERNEL;
      x.consumed = d.in.consumed;
      x.delivered = d.in.delivered;
      x.src_offset_in_block = d.in.off0;
      x.wire_len = d.wire_len;
      x.npkts = d.npk;
      continue;
    }
    out.note(fallback(x, b, proto, chunk_size, ctype, st));
  }
  return out.result();
}

}  // namespace
}  // namespace hdfs_relay_batch

using namespace hdfs_relay_batch;

extern "C" {

int hdfs_relay_batch_abi_version(void) { return HDFS_RELAY_BATCH_ABI_VERSION; }

const char *hdfs_relay_batch_last_error(void) { return hdfs_companion::last_error(); }

int hdfs_relay_batch_relay(hdfs_relay_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                           void *stream) {
  return relay(e, n, proto, chunk_size, ctype, stream, false, 0u, 0, nullptr);
}

int hdfs_relay_batch_layout(uint64_t payload, int64_t offset_in_block, int proto, int ctype, int finish,
                            uint64_t *wire_len, uint64_t *npkts) {
  if (wire_len) *wire_len = 0;
  if (npkts) *npkts = 0;
  if (!wire_len || !npkts) return hdfs_companion::fail(HDFS_CRC32C_EINVAL, "wire_len and npkts are needed");
  hdfs_wire::Layout L;
  const int rc = layout_write(payload, offset_in_block, 0, proto, ctype, finish != 0, L);
  if (rc) return rc;
  *wire_len = L.wire_len;
  *npkts = L.plan.size();
  return HDFS_CRC32C_OK;
}

int hdfs_relay_batch_time(hdfs_relay_batch_entry *e, size_t n, int proto, uint32_t chunk_size, int ctype,
                          unsigned flags, int iters, double *ms_per_iter) {
  return relay(e, n, proto, chunk_size, ctype, nullptr, true, flags, iters, ms_per_iter);
}

}  // extern "C"
