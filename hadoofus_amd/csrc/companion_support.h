// Host support shared by the fifteen companion libraries of
// libhadoofus_crc32c.so (md5crc.cpp, writev.cpp, the seven wire-stream
// libraries wire*.cpp and the six read-side libraries, which add
// read_batch_host.h): the last-error text, the engine's device, grow-only
// buffers, a device table with its pinned staging twin, scratch bound to a
// device with the two events of a timing call, where a pointer lives, the
// overlap sweep over the buffers of a batch, the packet argument check and the
// "always synchronise, then report" tail of a call.  Host only: no kernel file
// includes it.  Every library's export map keeps all of this local, so each
// library has its own copy, its own last-error text included.
#ifndef HADOOFUS_COMPANION_SUPPORT_H
#define HADOOFUS_COMPANION_SUPPORT_H

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hadoofus_crc32c.h"

namespace hdfs_companion {

// ---- last error -----------------------------------------------------------------
inline thread_local char g_err[512] = "";

// Stores the calling thread's last-error text and returns code.
__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

inline const char *last_error() { return g_err; }

// A failure of the main library is this call's failure, with its text.
inline int engine_fail(int rc, const char *what) { return fail(rc, "%s: %s", what, hdfs_crc32c_last_error()); }

// The failure just recorded gets a prefix ("entry 3", say): "<prefix>: <text>".
__attribute__((format(printf, 2, 3))) inline int prefix_fail(int rc, const char *fmt, ...) {
  char prefix[sizeof(g_err)], both[2 * sizeof(g_err) + 2];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(prefix, sizeof(prefix), fmt, ap);
  va_end(ap);
  snprintf(both, sizeof(both), "%s: %s", prefix, g_err);
  both[sizeof(g_err) - 1] = 0;  // cut at the end, as every text is
  std::memcpy(g_err, both, sizeof(g_err));
  return rc;
}

// ---- the engine's device --------------------------------------------------------
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

// The device the main library is bound to, initialising it if need be.
inline int engine_device(int *dev) {
  int rc = hdfs_crc32c_init(-1);
  if (rc == HDFS_CRC32C_OK) rc = hdfs_crc32c_bound_device(dev, nullptr, 0);
  return rc ? engine_fail(rc, "engine") : HDFS_CRC32C_OK;
}

// ---- grow-only buffers ------------------------------------------------------------
// Grown on demand to max(bytes, floor), never shrunk, kept between calls; freed
// means {null, 0}.  Alloc records the failure's text and returns its code.
template <int (*Alloc)(void **, size_t), void (*Free)(void *)>
struct GrowOnly {
  void *p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes, size_t floor) {
    if (bytes <= cap) return HDFS_CRC32C_OK;
    release();
    const size_t want = bytes < floor ? floor : bytes;
    const int rc = Alloc(&p, want);
    if (rc) {
      p = nullptr;
      return rc;
    }
    cap = want;
    return HDFS_CRC32C_OK;
  }
  void release() {
    if (p) Free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T *as() const {
    return static_cast<T *>(p);
  }
};

inline int device_alloc(void **p, size_t n) {
  if (hipMalloc(p, n) == hipSuccess) return HDFS_CRC32C_OK;
  (void)hipGetLastError();  // not sticky: the next call starts clean
  return fail(HDFS_CRC32C_ENOMEM, "device allocation of %zu bytes failed", n);
}
inline void device_free(void *p) { (void)hipFree(p); }

inline int pinned_alloc(void **p, size_t n) {
  if (hipHostMalloc(p, n, hipHostMallocDefault) == hipSuccess) return HDFS_CRC32C_OK;
  (void)hipGetLastError();
  return fail(HDFS_CRC32C_ENOMEM, "pinned allocation of %zu bytes failed", n);
}
inline void pinned_free(void *p) { (void)hipHostFree(p); }

using DeviceBuffer = GrowOnly<device_alloc, device_free>;
// The pinned-host twin; the allocator is a parameter (writev.cpp's is the
// engine's pin registry).
template <int (*Alloc)(void **, size_t) = pinned_alloc, void (*Free)(void *) = pinned_free>
using PinnedBuffer = GrowOnly<Alloc, Free>;

constexpr size_t kScratchFloor = size_t(64) << 10;
constexpr size_t kTableFloor = size_t(16) << 10;

// A device table and its pinned staging twin, grown together: a call fills
// pin and uploads it to dev.  A failure leaves both freed.
struct TablePair {
  DeviceBuffer dev;
  PinnedBuffer<> pin;
  int reserve(size_t bytes, size_t floor) {
    if (bytes <= dev.cap) return HDFS_CRC32C_OK;
    release();  // both go before either comes back
    if (dev.reserve(bytes, floor) || pin.reserve(bytes, floor)) {
      release();
      return fail(HDFS_CRC32C_ENOMEM, "allocation of %zu table bytes failed", bytes < floor ? floor : bytes);
    }
    return HDFS_CRC32C_OK;
  }
  void release() {
    dev.release();
    pin.release();
  }
};

// ---- scratch bound to a device ------------------------------------------------------
// The base of a library's scratch: the device it was built on, a blocking
// stream of its own (ordered after work queued earlier on the NULL stream) and
// the two events of a timing call.  The library adds its buffers and says how
// to free them.
struct DeviceScratch {
  int dev = -1;
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};  // created when a timing call first runs

  // Bound to device `to` (the current one) afterwards.  When it was bound to
  // another device, everything is released there first.  `what` names the
  // failure ("<what>: <the runtime's text>").
  template <class ReleaseOwn>
  int bind(int to, const char *what, ReleaseOwn &&release_own) {
    if (dev == to) return HDFS_CRC32C_OK;
    if (dev >= 0) {
      DeviceGuard g(dev);
      unbind(release_own);
    }
    const hipError_t e = hipStreamCreate(&st);
    if (e != hipSuccess) {
      st = nullptr;
      return fail(HDFS_CRC32C_EHIP, "%s: %s", what, hipGetErrorString(e));
    }
    dev = to;
    return HDFS_CRC32C_OK;
  }

  // Synchronise, free the library's buffers, then the events and the stream:
  // unbound.
  template <class ReleaseOwn>
  void unbind(ReleaseOwn &&release_own) {
    if (st) (void)hipStreamSynchronize(st);
    release_own();
    destroy_events();
    if (st) (void)hipStreamDestroy(st);
    st = nullptr;
    dev = -1;
  }

  // Both events exist afterwards.  A failure keeps neither: the next call
  // tries again.
  int timing_events() {
    if (ev[0]) return HDFS_CRC32C_OK;
    hipError_t e = hipEventCreate(&ev[0]);
    if (e != hipSuccess) ev[0] = nullptr;
    if (e == hipSuccess && (e = hipEventCreate(&ev[1])) != hipSuccess) {
      ev[1] = nullptr;
      destroy_events();  // a lone first event would pass for the pair
    }
    if (e == hipSuccess) return HDFS_CRC32C_OK;
    (void)hipGetLastError();
    return fail(HDFS_CRC32C_EHIP, "events: %s", hipGetErrorString(e));
  }

  void destroy_events() {
    for (hipEvent_t &e : ev) {
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
};

// ---- where a pointer lives ------------------------------------------------------------
struct Placement {
  enum Kind { kUnknown, kHost, kDevice };  // kUnknown: the runtime does not know the address
  Kind kind = kUnknown;
  int device = -1;
  void *device_ptr = nullptr;  // NULL: no kernel can reach it
  uintptr_t lo = 0, hi = 0;    // the allocation [lo, hi); 0, 0: not asked for or not found
};

// The allocation's range is asked for only where p is memory of device
// range_on_dev (-1: never).
inline Placement placement(const void *p, int range_on_dev = -1) {
  Placement w;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return w;
  }
  w.kind = a.type == hipMemoryTypeDevice ? Placement::kDevice : Placement::kHost;
  w.device = a.device;
  w.device_ptr = a.devicePointer;
  if (w.kind == Placement::kDevice && a.device == range_on_dev) {
    void *ab = nullptr;
    size_t as = 0;
    if (hipMemGetAddressRange(&ab, &as, const_cast<void *>(p)) != hipSuccess) {
      (void)hipGetLastError();
    } else {
      w.lo = reinterpret_cast<uintptr_t>(ab);
      w.hi = w.lo + as;
    }
  }
  return w;
}

inline int past_the_end(const void *p, uint64_t n, const char *what) {
  return fail(HDFS_CRC32C_EINVAL, "%s: %llu bytes at %p run past the end of their device allocation", what,
              (unsigned long long)n, p);
}

// [p, p + n) inside one allocation of device `dev`.  alloc_lo / alloc_hi (may
// be NULL): that allocation's address range, for a caller that checks many
// ranges of one allocation.
inline int device_range(const void *p, uint64_t n, int dev, const char *what, uintptr_t *alloc_lo = nullptr,
                        uintptr_t *alloc_hi = nullptr) {
  const Placement w = placement(p, dev);
  if (w.kind != Placement::kDevice) return fail(HDFS_CRC32C_EINVAL, "%s: %p is not device memory", what, p);
  if (w.device != dev)
    return fail(HDFS_CRC32C_EINVAL, "%s: memory of device %d, the engine runs on device %d", what, w.device, dev);
  if (!w.hi) return fail(HDFS_CRC32C_EINVAL, "%s: no device allocation at %p", what, p);
  const uintptr_t b = reinterpret_cast<uintptr_t>(p);
  if (b < w.lo || b > w.hi || n > w.hi - b) return past_the_end(p, n, what);
  if (alloc_lo) *alloc_lo = w.lo;
  if (alloc_hi) *alloc_hi = w.hi;
  return HDFS_CRC32C_OK;
}

// device_range asks the runtime about every pointer; the ranges of a batch
// mostly share a few allocations, so the allocations found so far answer first.
struct Allocations {
  struct A {
    uintptr_t lo, hi;
  };
  A seen[64];
  size_t nseen = 0;
  int check(const void *p, uint64_t n, int dev, const char *what) {
    const uintptr_t b = reinterpret_cast<uintptr_t>(p);
    for (size_t i = 0; i < nseen; i++)
      if (b >= seen[i].lo && b < seen[i].hi) return n > seen[i].hi - b ? past_the_end(p, n, what) : HDFS_CRC32C_OK;
    A a{0, 0};
    const int rc = device_range(p, n, dev, what, &a.lo, &a.hi);
    if (rc == HDFS_CRC32C_OK && nseen < 64) seen[nseen++] = a;
    return rc;
  }
};

// Of a gather write: every non-empty fragment inside one allocation of device
// `dev`, the stream inside one, and the stream clear of every fragment.
inline int check_places(const hdfs_crc32c_iovec *iov, int n, const void *wire, uint64_t wire_len, int dev) {
  int rc;
  Allocations al;
  const uintptr_t w0 = reinterpret_cast<uintptr_t>(wire), w1 = w0 + uintptr_t(wire_len);
  for (int i = 0; i < n; i++) {
    if (!iov[i].len) continue;
    if ((rc = al.check(iov[i].base, iov[i].len, dev, "data"))) return prefix_fail(rc, "fragment %d", i);
  }
  if ((rc = al.check(wire, wire_len, dev, "wire"))) return rc;
  for (int i = 0; i < n; i++) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(iov[i].base);
    if (iov[i].len && a < w1 && w0 < a + uintptr_t(iov[i].len))
      return fail(HDFS_CRC32C_EINVAL, "fragment %d and wire overlap", i);
  }
  return HDFS_CRC32C_OK;
}

// ---- the buffers of a batch: no writer over another writer or over any reader --------------
// A batch names ranges a kernel writes (a write's stream, a read's destination)
// and ranges it only reads (a write's data, a read's stream).  No written range
// may overlap another written range or a read one; read ranges may overlap each
// other.  The intervals sorted by their first byte, then one pass that remembers
// the furthest end among the written and among the read ranges seen so far.
struct Span {
  uintptr_t lo, hi;  // [lo, hi), not empty
  uint32_t k;        // entry
  uint32_t wire;     // 1: a written range
};

// The sweep's order; a caller with very many spans may hand them over in it.
inline bool span_before(const Span &a, const Span &b) {
  return a.lo != b.lo ? a.lo < b.lo : (a.wire != b.wire ? a.wire > b.wire : a.k < b.k);
}

// The two nouns of a refusal: "entry 3: <writer> overlaps the <writer|reader> of entry 1".
struct SpanNouns {
  const char *writer = "wire", *reader = "data";
};

// The sweep itself.  next() hands over the spans in the sweep's order, NULL at
// the end.  hit_wire / hit_other (may be NULL): on a refusal, the written range
// and the range it overlaps, for a caller whose ranges are more than one per
// entry and who names the one at fault.
template <class Next>
int sweep_spans(Next next, Span *hit_wire, Span *hit_other, SpanNouns nouns) {
  const auto refuse = [&](const Span &wire, const Span &other, uint32_t a, uint32_t b) {
    if (hit_wire) *hit_wire = wire;
    if (hit_other) *hit_other = other;
    return fail(HDFS_CRC32C_EINVAL, "entry %u: %s overlaps the %s of entry %u", a, nouns.writer,
                other.wire ? nouns.writer : nouns.reader, b);
  };
  const Span *far_w = nullptr, *far_d = nullptr;
  while (const Span *s = next()) {
    // every span ahead of s starts at or below s->lo: it overlaps s iff it ends behind s->lo
    if (far_w && far_w->hi > s->lo)  // writer over writer: the later entry is the one refused
      return s->wire ? refuse(*far_w, *s, std::max(far_w->k, s->k), std::min(far_w->k, s->k))
                     : refuse(*far_w, *s, far_w->k, s->k);
    if (s->wire && far_d && far_d->hi > s->lo) return refuse(*s, *far_d, s->k, far_d->k);
    const Span *&far = s->wire ? far_w : far_d;
    if (!far || s->hi > far->hi) far = s;
  }
  return HDFS_CRC32C_OK;
}

inline void sort_spans(std::vector<Span> &v) {  // one pass where they come in the sweep's order already
  if (!std::is_sorted(v.begin(), v.end(), span_before)) std::sort(v.begin(), v.end(), span_before);
}

// Written and read ranges in one array.
inline int check_overlaps(std::vector<Span> &v, Span *hit_wire = nullptr, Span *hit_other = nullptr,
                          SpanNouns nouns = SpanNouns{}) {
  sort_spans(v);
  size_t i = 0;
  return sweep_spans([&] { return i < v.size() ? &v[i++] : nullptr; }, hit_wire, hit_other, nouns);
}

// The written ranges and the read ranges apart, as the read side collects them:
// each array is sorted only where it does not rise already (the ranges of a
// batch laid out in order cost a pass, not a sort), and the two are merged as
// the sweep goes, a written range ahead of a read one that starts at its byte.
inline int check_overlaps(std::vector<Span> &writers, std::vector<Span> &readers, Span *hit_wire = nullptr,
                          Span *hit_other = nullptr, SpanNouns nouns = SpanNouns{}) {
  sort_spans(writers);
  sort_spans(readers);
  size_t i = 0, j = 0;
  return sweep_spans(
      [&]() -> const Span * {
        if (i < writers.size() && (j >= readers.size() || !span_before(readers[j], writers[i]))) return &writers[i++];
        return j < readers.size() ? &readers[j++] : nullptr;
      },
      hit_wire, hit_other, nouns);
}

// ---- the arguments of a packet run -----------------------------------------------------
inline bool packet_args_ok(int proto, int ctype, int64_t offset_in_block) {
  if (proto != HDFS_CRC32C_PROTO_V1 && proto != HDFS_CRC32C_PROTO_V2) return fail(HDFS_CRC32C_EINVAL, "proto must be 1 or 2"), false;
  if (ctype != HDFS_CRC32C_CSUM_NULL && ctype != HDFS_CRC32C_CSUM_CRC32 && ctype != HDFS_CRC32C_CSUM_CRC32C)
    return fail(HDFS_CRC32C_EINVAL, "bad checksum type %d", ctype), false;
  if (offset_in_block < 0) return fail(HDFS_CRC32C_EINVAL, "negative block offset"), false;
  return true;
}

// ---- the end of a call -------------------------------------------------------------------
// Always synchronises, even after an error: the scratch must be out of use
// before the caller's lock goes.  Then the plan (may be NULL) is destroyed, and
// the call's result is the engine's rc, else the HIP error as "<what>: <text>".
inline int sync_and_report(hipStream_t st, hipError_t e, int rc, hdfs_crc32c_plan *plan, const char *what) {
  const hipError_t se = hipStreamSynchronize(st);
  if (e == hipSuccess) e = se;
  if (plan) hdfs_crc32c_plan_destroy(plan);
  if (rc) return rc;
  if (e != hipSuccess) return fail(HDFS_CRC32C_EHIP, "%s: %s", what, hipGetErrorString(e));
  return HDFS_CRC32C_OK;
}

}  // namespace hdfs_companion

#endif  // HADOOFUS_COMPANION_SUPPORT_H
