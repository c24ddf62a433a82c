// CPU self-test of the companion libraries' shared host support
// (hadoofus_amd/csrc/companion_support.h, grid_segments / timed_frame_run of
// wire_layout.h, the fused libraries' device state of wire_fused_host.h, the
// batch front end of wire_batch_layout.h and the read side's skeleton of
// read_batch_host.h) against a fake HIP runtime and a
// fake engine, both defined here: the program is not linked to the HIP
// runtime.  The fakes count and log every call, remember the current device
// and can be told to fail, so the checks cover what the GPU tests cannot:
// failed allocations, streams and events, a device change, the exact runtime
// calls of a warm call, and the code that a call reaches only once a device
// has been found (where the buffers of a batch lie).  Prints "N failures".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "companion_support.h"
#include "read_batch_host.h"
#include "wire_batch_layout.h"
#include "wire_fused_host.h"
#include "wire_layout.h"

using namespace hdfs_companion;

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      g_fail++;                                                    \
    }                                                              \
  } while (0)

// ---- the fake runtime ---------------------------------------------------------------
namespace {

struct Block {
  size_t size;
  int device;
  bool host;   // pinned host memory the runtime knows
  bool owned;  // malloc'd here (the others are made-up addresses, never touched)
};

struct Fake {
  int cur = 0;                          // the current device
  std::map<uintptr_t, Block> blocks;    // live allocations by base
  std::map<std::string, int> n;         // calls by name
  std::vector<std::string> log;         // calls in order, with the device they ran on
  int calls = 0;                        // all runtime calls
  hipError_t sticky = hipSuccess;
  int fail_malloc = 0, fail_host_malloc = 0, fail_stream = 0, fail_sync = 0, fail_range = 0, fail_launch = 0;
  int fail_event = 0;  // n > 0: the n-th hipEventCreate from now fails
  int fail_async = 0;  // n > 0: the n-th hipMemcpyAsync from now fails
  struct Copy {
    const void *dst, *src;
    size_t n;
    hipMemcpyKind kind;
  };
  std::vector<Copy> copies;  // what hipMemcpyAsync was given; nothing is copied
  int events = 0;      // live events
  int cus = 256;       // hipDeviceGetAttribute's answer
  size_t copied = 0;   // bytes of the last hipMemcpy
  bool any_range = false;  // an address inside no block is reported as part of the lowest block
  int wrong_device_frees = 0, streams = 0;
  // the fake engine
  int init_rc = 0, bound_rc = 0, exec_rc = 0, engine_dev = 0, plans_destroyed = 0;
  std::string engine_text = "engine text";
  // hdfs_crc32c_read_packets: a stream of read_records records, as many written as there is room for
  struct Read {
    const void *stream;
    uint64_t len;
    int64_t client_offset, read_len;
    const hdfs_crc32c_iovec *iov;
    int iovcnt;
    hdfs_crc32c_packet *pkts;
    size_t room;
  };
  std::vector<Read> reads;
  size_t read_records = 0;
  int read_rc = 0;
  // hdfs_crc32c_parse_packets: one scripted piece per call
  struct Piece {
    int rc;
    size_t np;
    uint64_t used;
    bool ends;  // its last record is the empty last packet
  };
  struct Parse {
    const void *stream;
    uint64_t len;
    size_t room;
  };
  std::vector<Piece> pieces;
  std::vector<Parse> parses;

  void called(const char *name) {
    calls++;
    n[name]++;
    log.push_back(std::string(name) + "@" + std::to_string(cur));
  }
  const Block *find(uintptr_t p, uintptr_t *base) const {
    auto it = blocks.upper_bound(p);
    if (it == blocks.begin()) return nullptr;
    --it;
    if (p - it->first >= it->second.size) return nullptr;
    *base = it->first;
    return &it->second;
  }
  hipError_t failed(hipError_t e) { return sticky = e; }
} F;

struct FakeStream {
  int device;
};
struct FakeEvent {
  int device;
};

hipError_t fake_alloc(void **p, size_t n, bool host, const char *name, int &fail_flag) {
  F.called(name);
  if (fail_flag) {
    fail_flag--;
    *p = reinterpret_cast<void *>(uintptr_t(0xBAD));  // a careless caller would free this
    return F.failed(hipErrorOutOfMemory);
  }
  *p = std::malloc(n);
  F.blocks[reinterpret_cast<uintptr_t>(*p)] = Block{n, F.cur, host, true};
  return hipSuccess;
}

hipError_t fake_free(void *p, const char *name) {
  F.called(name);
  auto it = F.blocks.find(reinterpret_cast<uintptr_t>(p));
  if (it == F.blocks.end()) return F.failed(hipErrorInvalidValue);
  if (it->second.device != F.cur) F.wrong_device_frees++;
  if (it->second.owned) std::free(p);
  F.blocks.erase(it);
  return hipSuccess;
}

// A device or host block at a made-up address.
void fake_block(uintptr_t base, size_t size, int device, bool host = false) {
  F.blocks[base] = Block{size, device, host, false};
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void **p, size_t n) { return fake_alloc(p, n, false, "hipMalloc", F.fail_malloc); }
hipError_t hipFree(void *p) { return fake_free(p, "hipFree"); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return fake_alloc(p, n, true, "hipHostMalloc", F.fail_host_malloc); }
hipError_t hipHostFree(void *p) { return fake_free(p, "hipHostFree"); }
hipError_t hipGetDevice(int *d) {
  F.called("hipGetDevice");
  *d = F.cur;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) {
  F.cur = d;
  F.called("hipSetDevice");
  return hipSuccess;
}
hipError_t hipStreamCreate(hipStream_t *s) {
  F.called("hipStreamCreate");
  if (F.fail_stream) {
    F.fail_stream--;
    *s = reinterpret_cast<hipStream_t>(uintptr_t(0xBAD));
    return F.failed(hipErrorOutOfMemory);
  }
  F.streams++;
  *s = reinterpret_cast<hipStream_t>(new FakeStream{F.cur});
  return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
  F.called("hipStreamSynchronize");
  if (F.fail_sync) {
    F.fail_sync--;
    return F.failed(hipErrorLaunchFailure);
  }
  return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
  F.called("hipStreamDestroy");
  FakeStream *fs = reinterpret_cast<FakeStream *>(s);
  if (fs->device != F.cur) F.wrong_device_frees++;
  delete fs;
  F.streams--;
  return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *a, const void *p) {
  F.called("hipPointerGetAttributes");
  uintptr_t base = 0;
  const Block *b = F.find(reinterpret_cast<uintptr_t>(p), &base);
  if (!b && F.any_range && !F.blocks.empty()) b = &F.blocks.begin()->second;
  if (!b) return F.failed(hipErrorInvalidValue);
  std::memset(a, 0, sizeof(*a));
  a->type = b->host ? hipMemoryTypeHost : hipMemoryTypeDevice;
  a->device = b->device;
  a->devicePointer = const_cast<void *>(p);
  a->hostPointer = b->host ? const_cast<void *>(p) : nullptr;
  return hipSuccess;
}
hipError_t hipMemGetAddressRange(hipDeviceptr_t *pbase, size_t *psize, hipDeviceptr_t p) {
  F.called("hipMemGetAddressRange");
  uintptr_t base = 0;
  const Block *b = F.find(reinterpret_cast<uintptr_t>(p), &base);
  if (!b && F.any_range && !F.blocks.empty()) {
    base = F.blocks.begin()->first;
    b = &F.blocks.begin()->second;
  }
  if (!b || F.fail_range) return F.failed(hipErrorInvalidValue);
  *pbase = reinterpret_cast<hipDeviceptr_t>(base);
  *psize = b->size;
  return hipSuccess;
}
hipError_t hipGetLastError(void) {
  F.called("hipGetLastError");
  const hipError_t e = F.sticky;
  F.sticky = hipSuccess;
  return e;
}
const char *hipGetErrorString(hipError_t e) {
  return e == hipErrorOutOfMemory ? "fake: out of memory" : e == hipErrorLaunchFailure ? "fake: launch failure" : "fake: error";
}
hipError_t hipEventCreate(hipEvent_t *e) {
  F.called("hipEventCreate");
  if (F.fail_event && !--F.fail_event) {
    *e = reinterpret_cast<hipEvent_t>(uintptr_t(0xBAD));  // a careless caller would destroy this
    return F.failed(hipErrorOutOfMemory);
  }
  F.events++;
  *e = reinterpret_cast<hipEvent_t>(new FakeEvent{F.cur});
  return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
  F.called("hipEventDestroy");
  FakeEvent *fe = reinterpret_cast<FakeEvent *>(e);
  if (fe->device != F.cur) F.wrong_device_frees++;
  delete fe;
  F.events--;
  return hipSuccess;
}
hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind) {
  F.called("hipMemcpy");
  uintptr_t base = 0;
  const Block *b = F.find(reinterpret_cast<uintptr_t>(dst), &base);
  if (!b || !b->owned || n > b->size - (reinterpret_cast<uintptr_t>(dst) - base)) return F.failed(hipErrorInvalidValue);
  std::memcpy(dst, src, n);
  F.copied = n;
  return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t) {
  F.called("hipMemcpyAsync");
  F.copies.push_back(Fake::Copy{dst, src, n, kind});
  return F.fail_async && !--F.fail_async ? F.failed(hipErrorOutOfMemory) : hipSuccess;
}
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t, int) {
  F.called("hipDeviceGetAttribute");
  *v = F.cus;
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) {
  F.called("hipEventRecord");
  return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t, hipEvent_t) {
  F.called("hipEventElapsedTime");
  *ms = 6.0f;
  return hipSuccess;
}

// ---- the fake engine ------------------------------------------------------------------
int hdfs_crc32c_init(int) {
  F.called("init");
  return F.init_rc;
}
int hdfs_crc32c_bound_device(int *dev, char *, size_t) {
  F.called("bound_device");
  if (!F.bound_rc) *dev = F.engine_dev;
  return F.bound_rc;
}
const char *hdfs_crc32c_last_error(void) { return F.engine_text.c_str(); }
int hdfs_crc32c_plan_execute(hdfs_crc32c_plan *, void *) {
  F.called("plan_execute");
  return F.exec_rc;
}
int hdfs_crc32c_read_packets(const void *stream, uint64_t len, int, uint32_t, int, int64_t client_offset, int64_t read_len,
                             const hdfs_crc32c_iovec *iov, int iovcnt, hdfs_crc32c_packet *pkts, size_t max_pkts,
                             size_t *npkts, uint64_t *consumed, uint64_t *delivered) {
  F.called("read_packets");
  F.reads.push_back(Fake::Read{stream, len, client_offset, read_len, iov, iovcnt, pkts, max_pkts});
  if (F.read_rc < 0) return F.read_rc;
  *npkts = std::min(max_pkts, F.read_records);
  for (size_t i = 0; i < *npkts; i++) pkts[i].offset_in_block = int64_t(1000 + i);  // the room is really there
  *consumed = len;
  *delivered = 77;
  return F.read_rc;
}
int hdfs_crc32c_parse_packets(const void *stream, uint64_t len, int, uint32_t, int, hdfs_crc32c_packet *pkts,
                              size_t max_pkts, size_t *npkts, uint64_t *consumed) {
  F.called("parse_packets");
  const Fake::Piece p = F.pieces.at(F.parses.size());
  F.parses.push_back(Fake::Parse{stream, len, max_pkts});
  if (p.rc < 0) return p.rc;
  if (p.np > max_pkts) std::abort();
  for (size_t i = 0; i < p.np; i++) {
    pkts[i] = hdfs_crc32c_packet{};
    pkts[i].stream_off = 100 * i;
    pkts[i].offset_in_block = int64_t(4096 + len);  // another one in every piece
    pkts[i].data_len = 10;
    pkts[i].crc_len = 4;
    pkts[i].header_len = 31;
  }
  if (p.np && p.rc > 0) pkts[p.np - 1].error = p.rc;
  if (p.np && p.ends) pkts[p.np - 1].data_len = pkts[p.np - 1].crc_len = 0;
  *npkts = p.np;
  *consumed = p.used;
  return p.rc;
}
void hdfs_crc32c_plan_destroy(hdfs_crc32c_plan *) {
  F.called("plan_destroy");
  F.plans_destroyed++;
}
}  // extern "C"

namespace {

hdfs_crc32c_plan *const kPlan = reinterpret_cast<hdfs_crc32c_plan *>(uintptr_t(0x5150));

std::string names_since(size_t from) {  // "a b c": the calls logged since, without their devices
  std::string s;
  for (size_t i = from; i < F.log.size(); i++) s += (s.empty() ? "" : " ") + F.log[i].substr(0, F.log[i].find('@'));
  return s;
}

bool err_is(const char *want) {
  if (!std::strcmp(last_error(), want)) return true;
  std::printf("  last error: \"%s\"\n  wanted:     \"%s\"\n", last_error(), want);
  return false;
}

// ---- last error ---------------------------------------------------------------------------
void test_last_error() {
  CHECK(fail(-7, "a %d b %s", 5, "c") == -7 && err_is("a 5 b c"));
  const std::string big(600, 'x');
  CHECK(fail(-1, "%s", big.c_str()) == -1);
  CHECK(std::strlen(last_error()) == 511 && std::string(last_error()) == big.substr(0, 511));
  // a prefix in front of a text that is already full: still 511 bytes, the text cut at the end
  CHECK(prefix_fail(-3, "entry %zu", size_t(7)) == -3);
  CHECK(std::strlen(last_error()) == 511 && std::string(last_error()) == "entry 7: " + big.substr(0, 502));
  fail(-1, "negative block offset");
  CHECK(prefix_fail(-1, "entry %zu", size_t(65535)) == -1 && err_is("entry 65535: negative block offset"));
  fail(-1, "%s", "");
  CHECK(prefix_fail(-2, "p") == -2 && err_is("p: "));
  F.engine_text = "no device";
  CHECK(engine_fail(-4, "compute plan") == -4 && err_is("compute plan: no device"));
  // every thread has its own text
  fail(-1, "main thread");
  std::string seen[2];
  std::vector<std::thread> th;
  for (int t = 0; t < 2; t++)
    th.emplace_back([t, &seen] {
      CHECK(last_error()[0] == 0);  // a new thread starts empty
      for (int i = 0; i < 2000; i++) fail(-1, "thread %d round %d", t, i);
      seen[t] = last_error();
    });
  for (auto &t : th) t.join();
  CHECK(seen[0] == "thread 0 round 1999" && seen[1] == "thread 1 round 1999" && err_is("main thread"));
}

void test_engine_device() {
  int dev = -1;
  F.engine_dev = 3;
  size_t at = F.log.size();
  CHECK(engine_device(&dev) == 0 && dev == 3 && names_since(at) == "init bound_device");
  F.init_rc = -6;
  F.engine_text = "no GPU";
  at = F.log.size();
  CHECK(engine_device(&dev) == -6 && err_is("engine: no GPU") && names_since(at) == "init");
  F.init_rc = 0;
  F.bound_rc = -2;
  CHECK(engine_device(&dev) == -2 && err_is("engine: no GPU"));
  F.bound_rc = 0;
  F.engine_dev = 0;
}

// ---- grow-only buffers -----------------------------------------------------------------------
int g_custom_allocs = 0, g_custom_frees = 0;
int custom_alloc(void **p, size_t n) {
  g_custom_allocs++;
  if (n > (size_t(1) << 20)) return fail(-9, "custom allocator: %zu bytes are too many", n);
  *p = std::malloc(n);
  return 0;
}
void custom_free(void *p) {
  g_custom_frees++;
  std::free(p);
}

template <class Buf>
void grow_only(Buf &b, const char *alloc, const char *free_, int &fail_flag, const char *enomem_fmt) {
  const std::string up = std::string(free_) + " " + alloc;
  CHECK(b.p == nullptr && b.cap == 0);
  size_t at = F.log.size();
  CHECK(b.reserve(0, 65536) == 0 && b.p == nullptr && F.log.size() == at);  // nothing asked, nothing done
  CHECK(b.reserve(1, 65536) == 0 && b.p && b.cap == 65536 && names_since(at) == alloc);  // the floor
  void *first = b.p;
  at = F.log.size();
  CHECK(b.reserve(65536, 65536) == 0 && b.reserve(17, 65536) == 0 && b.reserve(0, 65536) == 0);
  CHECK(F.log.size() == at && b.p == first && b.cap == 65536);  // within capacity: no runtime call
  CHECK(b.reserve(65537, 65536) == 0 && b.cap == 65537 && names_since(at) == up);  // one free, one allocation
  at = F.log.size();
  CHECK(b.reserve(100, 16384) == 0 && b.cap == 65537 && F.log.size() == at);  // never shrunk
  // a failed allocation: {null, 0}, ENOMEM, the text, the runtime's error cleared; the next call retries
  fail_flag = 1;
  CHECK(b.reserve(1 << 20, 65536) == HDFS_CRC32C_ENOMEM && b.p == nullptr && b.cap == 0);
  char want[128];
  std::snprintf(want, sizeof(want), enomem_fmt, size_t(1) << 20);
  CHECK(err_is(want) && F.sticky == hipSuccess && names_since(at) == up + " hipGetLastError");
  at = F.log.size();
  CHECK(b.reserve(5, 16384) == 0 && b.cap == 16384 && names_since(at) == alloc);  // another floor
  at = F.log.size();
  b.release();
  CHECK(b.p == nullptr && b.cap == 0 && names_since(at) == free_);
  b.release();
  CHECK(F.log.size() == at + 1);  // idempotent
}

void test_buffers() {
  const size_t live = F.blocks.size();
  DeviceBuffer d;
  grow_only(d, "hipMalloc", "hipFree", F.fail_malloc, "device allocation of %zu bytes failed");
  PinnedBuffer<> h;
  grow_only(h, "hipHostMalloc", "hipHostFree", F.fail_host_malloc, "pinned allocation of %zu bytes failed");
  CHECK(F.blocks.size() == live && F.wrong_device_frees == 0);
  // the pinned twin with another allocator: its code and its text
  const int calls = F.calls;
  PinnedBuffer<custom_alloc, custom_free> c;
  CHECK(c.reserve(10, 65536) == 0 && c.cap == 65536 && c.reserve(65536, 65536) == 0 && g_custom_allocs == 1);
  CHECK(c.reserve(2 << 20, 65536) == -9 && c.p == nullptr && c.cap == 0 && g_custom_frees == 1);
  CHECK(err_is("custom allocator: 2097152 bytes are too many"));
  CHECK(c.reserve(70000, 65536) == 0 && c.cap == 70000 && g_custom_allocs == 3 && g_custom_frees == 1);
  c.release();
  c.release();
  CHECK(g_custom_frees == 2 && F.calls == calls);  // no runtime call at all
}

// ---- scratch bound to a device ---------------------------------------------------------------
struct TestScratch : DeviceScratch {
  DeviceBuffer a, b;
  int released = 0;
  int reserve(int to, size_t bytes) {
    const int rc = bind(to, "stream", [this] {
      released++;
      a.release();
      b.release();
    });
    if (rc) return rc;
    return a.reserve(bytes, 65536) || b.reserve(bytes, 16384) ? HDFS_CRC32C_ENOMEM : HDFS_CRC32C_OK;
  }
};

void test_scratch() {
  const size_t live = F.blocks.size();
  TestScratch s;
  F.cur = 0;
  size_t at = F.log.size();
  CHECK(s.reserve(0, 100) == 0 && s.dev == 0 && s.st && F.streams == 1);
  CHECK(names_since(at) == "hipStreamCreate hipMalloc hipMalloc" && s.released == 0);
  at = F.log.size();
  CHECK(s.reserve(0, 100) == 0 && F.log.size() == at);  // a warm call: no runtime call
  // the engine moved to device 2; the caller made it current, as the libraries do (DeviceGuard)
  F.cur = 2;
  at = F.log.size();
  CHECK(s.reserve(2, 100) == 0 && s.dev == 2 && s.released == 1 && F.streams == 1 && F.cur == 2);
  std::string got;
  for (size_t i = at; i < F.log.size(); i++) got += F.log[i] + " ";
  // synchronised and freed on the old device, the caller's device restored, rebuilt on the new one
  CHECK(got == "hipGetDevice@2 hipSetDevice@0 hipStreamSynchronize@0 hipFree@0 hipFree@0 hipStreamDestroy@0 "
               "hipSetDevice@2 hipStreamCreate@2 hipMalloc@2 hipMalloc@2 ");
  CHECK(F.wrong_device_frees == 0 && reinterpret_cast<FakeStream *>(s.st)->device == 2);
  // a failed stream creation: unbound, nothing kept; the next call retries
  F.cur = 1;
  F.fail_stream = 1;
  CHECK(s.reserve(1, 100) == HDFS_CRC32C_EHIP && err_is("stream: fake: out of memory"));
  CHECK(s.dev == -1 && s.st == nullptr && s.a.p == nullptr && s.b.p == nullptr && F.streams == 0 && F.cur == 1);
  CHECK(s.released == 2 && F.wrong_device_frees == 0);
  at = F.log.size();
  CHECK(s.reserve(1, 100) == 0 && s.dev == 1 && names_since(at) == "hipStreamCreate hipMalloc hipMalloc");
  // a failed allocation leaves the binding; the next call retries the buffer alone
  F.fail_malloc = 1;
  CHECK(s.reserve(1, 1 << 20) == HDFS_CRC32C_ENOMEM && s.dev == 1 && s.st && s.a.p == nullptr);
  at = F.log.size();
  CHECK(s.reserve(1, 1 << 20) == 0 && names_since(at) == "hipMalloc hipFree hipMalloc");
  at = F.log.size();
  s.unbind([&] {
    s.a.release();
    s.b.release();
  });
  CHECK(names_since(at) == "hipStreamSynchronize hipFree hipFree hipStreamDestroy" && s.dev == -1 && !s.st);
  at = F.log.size();
  s.unbind([] {});
  CHECK(F.log.size() == at && F.blocks.size() == live && F.streams == 0);
  F.cur = 0;
  // DeviceGuard alone: no set when the device is current already
  at = F.log.size();
  { DeviceGuard g(0); }
  CHECK(names_since(at) == "hipGetDevice");
  { DeviceGuard g(5); CHECK(F.cur == 5); }
  CHECK(F.cur == 0);
}

// ---- the two events of a timing call -----------------------------------------------------------
void test_timing_events() {
  TestScratch s;
  F.cur = 0;
  CHECK(s.reserve(0, 100) == 0 && !s.ev[0] && !s.ev[1]);
  size_t at = F.log.size();
  CHECK(s.timing_events() == 0 && s.ev[0] && s.ev[1] && F.events == 2);
  CHECK(names_since(at) == "hipEventCreate hipEventCreate");  // created on first use
  at = F.log.size();
  CHECK(s.timing_events() == 0 && s.reserve(0, 100) == 0 && F.log.size() == at);  // a warm call: no runtime call
  // a device change: destroyed once, behind the library's buffers and ahead of the stream, the old device current
  F.cur = 2;
  at = F.log.size();
  CHECK(s.reserve(2, 100) == 0 && F.events == 0 && !s.ev[0] && !s.ev[1] && F.wrong_device_frees == 0);
  std::string got;
  for (size_t i = at; i < F.log.size(); i++) got += F.log[i] + " ";
  CHECK(got == "hipGetDevice@2 hipSetDevice@0 hipStreamSynchronize@0 hipFree@0 hipFree@0 hipEventDestroy@0 "
               "hipEventDestroy@0 hipStreamDestroy@0 hipSetDevice@2 hipStreamCreate@2 hipMalloc@2 hipMalloc@2 ");
  // a failed create: EHIP, the text, the runtime's error cleared, nothing kept; the next call retries
  F.fail_event = 1;
  at = F.log.size();
  CHECK(s.timing_events() == HDFS_CRC32C_EHIP && err_is("events: fake: out of memory") && F.sticky == hipSuccess);
  CHECK(!s.ev[0] && !s.ev[1] && F.events == 0 && names_since(at) == "hipEventCreate hipGetLastError");
  // ... and of the second event: the first does not pass for the pair
  F.fail_event = 2;
  at = F.log.size();
  CHECK(s.timing_events() == HDFS_CRC32C_EHIP && err_is("events: fake: out of memory") && F.sticky == hipSuccess);
  CHECK(!s.ev[0] && !s.ev[1] && F.events == 0);
  CHECK(names_since(at) == "hipEventCreate hipEventCreate hipEventDestroy hipGetLastError");
  at = F.log.size();
  CHECK(s.timing_events() == 0 && s.ev[0] && s.ev[1] && F.events == 2);
  CHECK(names_since(at) == "hipEventCreate hipEventCreate");
  at = F.log.size();
  s.unbind([&] {
    s.a.release();
    s.b.release();
  });
  CHECK(names_since(at) == "hipStreamSynchronize hipFree hipFree hipEventDestroy hipEventDestroy hipStreamDestroy");
  CHECK(F.events == 0 && F.streams == 0 && F.wrong_device_frees == 0);
  F.cur = 0;
}

// ---- a device table and its pinned twin --------------------------------------------------------
void test_table_pair() {
  const size_t live = F.blocks.size();
  auto empty = [](const TablePair &t) { return !t.dev.p && !t.dev.cap && !t.pin.p && !t.pin.cap; };
  CHECK(kTableFloor == 16384 && kScratchFloor == 65536);
  TablePair t;
  size_t at = F.log.size();
  CHECK(t.reserve(0, kTableFloor) == 0 && empty(t) && F.log.size() == at);  // nothing asked, nothing done
  CHECK(t.reserve(1, kTableFloor) == 0 && t.dev.p && t.pin.p && t.dev.cap == 16384 && t.pin.cap == 16384);
  CHECK(names_since(at) == "hipMalloc hipHostMalloc");  // the floor
  const void *d0 = t.dev.p, *p0 = t.pin.p;
  at = F.log.size();
  CHECK(t.reserve(16384, kTableFloor) == 0 && t.reserve(5, kTableFloor) == 0 && t.reserve(0, kTableFloor) == 0);
  CHECK(F.log.size() == at && t.dev.p == d0 && t.pin.p == p0);  // within capacity: no runtime call
  CHECK(t.reserve(16385, kTableFloor) == 0 && t.dev.cap == 16385 && t.pin.cap == 16385);
  CHECK(names_since(at) == "hipFree hipHostFree hipMalloc hipHostMalloc");  // both go before either comes back
  // the device side fails: both {null, 0}, ENOMEM, the text, the runtime's error cleared
  F.fail_malloc = 1;
  at = F.log.size();
  CHECK(t.reserve(1 << 20, kTableFloor) == HDFS_CRC32C_ENOMEM && empty(t) && F.sticky == hipSuccess);
  CHECK(err_is("allocation of 1048576 table bytes failed"));
  CHECK(names_since(at) == "hipFree hipHostFree hipMalloc hipGetLastError");
  at = F.log.size();
  CHECK(t.reserve(1 << 20, kTableFloor) == 0 && t.dev.cap == (1 << 20) && t.pin.cap == (1 << 20));  // the next call
  CHECK(names_since(at) == "hipMalloc hipHostMalloc");
  // the pinned side fails: the device table goes too
  F.fail_host_malloc = 1;
  at = F.log.size();
  CHECK(t.reserve((1 << 20) + 1, kTableFloor) == HDFS_CRC32C_ENOMEM && empty(t) && F.sticky == hipSuccess);
  CHECK(err_is("allocation of 1048577 table bytes failed"));
  CHECK(names_since(at) == "hipFree hipHostFree hipMalloc hipHostMalloc hipGetLastError hipFree");
  // the text counts what was asked of the runtime: max(bytes, floor)
  F.fail_malloc = 1;
  CHECK(t.reserve(100, kTableFloor) == HDFS_CRC32C_ENOMEM && empty(t) && err_is("allocation of 16384 table bytes failed"));
  at = F.log.size();
  CHECK(t.reserve(100, kTableFloor) == 0 && t.dev.cap == 16384 && names_since(at) == "hipMalloc hipHostMalloc");
  at = F.log.size();
  t.release();
  CHECK(empty(t) && names_since(at) == "hipFree hipHostFree");
  t.release();
  CHECK(F.log.size() == at + 2 && F.blocks.size() == live && F.wrong_device_frees == 0);
}

// ---- the fused libraries' device state ---------------------------------------------------------
int g_prepares = 0;
hipError_t g_prepare_rc = hipSuccess;
hipError_t counted_prepare() {
  F.called("prepare");
  g_prepares++;
  return g_prepare_rc;
}
using FusedState = hdfs_wire_fused::DeviceState<counted_prepare, 1024u>;

struct FusedScratch : DeviceScratch {  // as the three libraries build theirs
  FusedState fused;
  TablePair tab;
  int reserve(int to, size_t tab_bytes) {
    int rc = bind(to, "stream", [this] {
      fused.release();
      tab.release();
    });
    if (rc || (rc = fused.setup(to))) return rc;
    return tab.reserve(tab_bytes, kTableFloor);
  }
};

void test_fused_state() {
  namespace crc = hdfs_wire_fused::crc;
  const size_t live = F.blocks.size(), bytes = 2 * size_t(crc::kCompactWords) * sizeof(uint32_t);
  std::vector<uint32_t> want(2 * crc::kCompactWords);
  crc::make_compact(hdfs_crc32c::kPoly, want.data());
  crc::make_compact(hdfs_crc32c::kPolyZlib, want.data() + crc::kCompactWords);
  CHECK(std::memcmp(want.data(), want.data() + crc::kCompactWords, bytes / 2) != 0);
  const int cus[4] = {0, 1, 256, 5000};
  const uint32_t groups[4] = {1, 1, 256, 1024};
  for (int i = 0; i < 4; i++) {
    FusedState s;
    F.cus = cus[i];
    F.copied = 0;
    g_prepares = 0;
    size_t at = F.log.size();
    CHECK(s.setup(0) == 0 && s.ready && s.groups == groups[i] && g_prepares == 1);
    CHECK(names_since(at) == "hipMalloc hipMemcpy hipDeviceGetAttribute prepare");  // one upload, one prepare
    CHECK(F.copied == bytes && s.crc_tab.cap == bytes && !std::memcmp(s.crc_tab.p, want.data(), bytes));  // CRC32C first
    at = F.log.size();
    CHECK(s.setup(0) == 0 && F.log.size() == at && g_prepares == 1);  // a warm call: no runtime call
    CHECK(s.tables(HDFS_CRC32C_CSUM_CRC32C) == s.crc_tab.as<uint32_t>() && s.tables(HDFS_CRC32C_CSUM_NULL) == s.crc_tab.p);
    CHECK(s.tables(HDFS_CRC32C_CSUM_CRC32) == s.crc_tab.as<uint32_t>() + crc::kCompactWords);
    // the grid: a workgroup per CU and none without a packet, unless the flags ask for a number
    CHECK(s.grid(0u, 1) == 1 && s.grid(0u, groups[i]) == groups[i] && s.grid(0u, 70000) == groups[i]);
    CHECK(s.grid(7u << 8, 1) == 7 && s.grid(1024u << 8, 3) == 1024);
    s.release();
    CHECK(!s.ready && !s.crc_tab.p);
  }
  F.cus = 256;
  CHECK(FusedState::flags_ok(0u) == 0 && FusedState::flags_ok(1u << 8) == 0 && FusedState::flags_ok(1024u << 8) == 0);
  CHECK(FusedState::flags_ok(1025u << 8) == HDFS_CRC32C_EINVAL && err_is("1 to 1024 workgroups"));
  CHECK(FusedState::flags_ok((4u << 8) | 1u) == HDFS_CRC32C_EINVAL && err_is("1 to 1024 workgroups"));
  // in a scratch: a warm call makes no runtime call, a device change uploads and prepares again
  FusedScratch s;
  F.cur = 0;
  g_prepares = 0;
  size_t at = F.log.size();
  CHECK(s.reserve(0, 100) == 0 && g_prepares == 1);
  CHECK(names_since(at) == "hipStreamCreate hipMalloc hipMemcpy hipDeviceGetAttribute prepare hipMalloc hipHostMalloc");
  at = F.log.size();
  CHECK(s.reserve(0, 16384) == 0 && s.reserve(0, 0) == 0 && F.log.size() == at && g_prepares == 1);
  F.cur = 2;
  at = F.log.size();
  CHECK(s.reserve(2, 100) == 0 && g_prepares == 2 && s.fused.ready && F.wrong_device_frees == 0);
  std::string got;
  for (size_t i = at; i < F.log.size(); i++) got += F.log[i] + " ";
  CHECK(got == "hipGetDevice@2 hipSetDevice@0 hipStreamSynchronize@0 hipFree@0 hipFree@0 hipHostFree@0 "
               "hipStreamDestroy@0 hipSetDevice@2 hipStreamCreate@2 hipMalloc@2 hipMemcpy@2 hipDeviceGetAttribute@2 "
               "prepare@2 hipMalloc@2 hipHostMalloc@2 ");
  s.unbind([&] {
    s.fused.release();
    s.tab.release();
  });
  // a failing prepare: EHIP, the text, not ready; the next call uploads and prepares again
  FusedState f;
  g_prepare_rc = hipErrorLaunchFailure;
  CHECK(f.setup(2) == HDFS_CRC32C_EHIP && err_is("tables: fake: launch failure") && !f.ready);
  g_prepare_rc = hipSuccess;
  at = F.log.size();
  CHECK(f.setup(2) == 0 && f.ready && f.groups == 256 && names_since(at) == "hipMemcpy hipDeviceGetAttribute prepare");
  // a failed table allocation is the buffer's failure
  f.release();
  F.fail_malloc = 1;
  CHECK(f.setup(2) == HDFS_CRC32C_ENOMEM && !f.ready && F.sticky == hipSuccess);
  F.cur = 0;
  CHECK(F.blocks.size() == live && F.streams == 0 && F.wrong_device_frees == 0);
}

// ---- where a pointer lives ----------------------------------------------------------------------
void test_placement() {
  const uintptr_t A = 0x7000'0000'0000ull, B = 0x7100'0000'0000ull, H = 0x7200'0000'0000ull;
  auto ptr = [](uintptr_t a) { return reinterpret_cast<const void *>(a); };
  fake_block(A, 4096, 0);
  fake_block(B, 4096, 1);
  fake_block(H, 4096, 0, true);
  char want[256];
  size_t at = F.log.size();
  uintptr_t lo = 0, hi = 0;
  CHECK(device_range(ptr(A + 10), 100, 0, "data", &lo, &hi) == 0 && lo == A && hi == A + 4096);
  CHECK(names_since(at) == "hipPointerGetAttributes hipMemGetAddressRange");
  CHECK(device_range(ptr(A), 4096, 0, "data") == 0 && device_range(ptr(A + 4095), 1, 0, "data") == 0);
  CHECK(device_range(ptr(A + 4095), 0, 0, "data") == 0);
  CHECK(device_range(ptr(A + 4095), 2, 0, "wire") == HDFS_CRC32C_EINVAL);  // one past the end
  std::snprintf(want, sizeof(want), "wire: 2 bytes at %p run past the end of their device allocation", ptr(A + 4095));
  CHECK(err_is(want));
  CHECK(device_range(ptr(A + 10), UINT64_MAX, 0, "data") == HDFS_CRC32C_EINVAL);  // p + n wraps
  std::snprintf(want, sizeof(want), "data: %llu bytes at %p run past the end of their device allocation",
                (unsigned long long)UINT64_MAX, ptr(A + 10));
  CHECK(err_is(want));
  CHECK(device_range(ptr(A + 10), UINT64_MAX - 5, 0, "data") == HDFS_CRC32C_EINVAL);
  // the first byte behind the allocation: the runtime does not know it
  at = F.log.size();
  CHECK(device_range(ptr(A + 4096), 0, 0, "data") == HDFS_CRC32C_EINVAL);
  std::snprintf(want, sizeof(want), "data: %p is not device memory", ptr(A + 4096));
  CHECK(err_is(want) && names_since(at) == "hipPointerGetAttributes hipGetLastError" && F.sticky == hipSuccess);
  // ... and when the runtime does name an allocation for it: a zero-length
  // range at the very end is inside, anything else and anything further is not
  F.any_range = true;
  CHECK(device_range(ptr(A + 4096), 0, 0, "data") == 0);
  CHECK(device_range(ptr(A + 4096), 1, 0, "data") == HDFS_CRC32C_EINVAL);
  CHECK(device_range(ptr(A + 4097), 0, 0, "data") == HDFS_CRC32C_EINVAL);
  std::snprintf(want, sizeof(want), "data: 0 bytes at %p run past the end of their device allocation", ptr(A + 4097));
  CHECK(err_is(want));
  CHECK(device_range(ptr(A - 1), 1, 0, "data") == HDFS_CRC32C_EINVAL);
  F.any_range = false;
  // another device's memory: refused before its allocation is asked for
  at = F.log.size();
  CHECK(device_range(ptr(B + 8), 8, 0, "wire") == HDFS_CRC32C_EINVAL);
  CHECK(err_is("wire: memory of device 1, the engine runs on device 0") && names_since(at) == "hipPointerGetAttributes");
  CHECK(device_range(ptr(B + 8), 8, 1, "wire") == 0);
  // host memory the runtime knows, and memory it does not
  CHECK(device_range(ptr(H), 8, 0, "data") == HDFS_CRC32C_EINVAL);
  std::snprintf(want, sizeof(want), "data: %p is not device memory", ptr(H));
  CHECK(err_is(want));
  int local = 0;
  CHECK(device_range(&local, 4, 0, "data") == HDFS_CRC32C_EINVAL);
  F.fail_range = 1;
  CHECK(device_range(ptr(A), 1, 0, "data") == HDFS_CRC32C_EINVAL && F.sticky == hipSuccess);
  std::snprintf(want, sizeof(want), "data: no device allocation at %p", ptr(A));
  CHECK(err_is(want));
  F.fail_range = 0;
  // the query itself
  at = F.log.size();
  Placement w = placement(ptr(A + 1));
  CHECK(w.kind == Placement::kDevice && w.device == 0 && w.device_ptr == ptr(A + 1) && w.lo == 0 && w.hi == 0);
  CHECK(names_since(at) == "hipPointerGetAttributes");  // no range unless asked for
  w = placement(ptr(A + 1), 0);
  CHECK(w.kind == Placement::kDevice && w.lo == A && w.hi == A + 4096);
  w = placement(ptr(B), 0);
  CHECK(w.kind == Placement::kDevice && w.device == 1 && w.hi == 0);
  w = placement(ptr(H + 5), 0);
  CHECK(w.kind == Placement::kHost && w.device_ptr == ptr(H + 5) && w.hi == 0);
  w = placement(&local, 0);
  CHECK(w.kind == Placement::kUnknown && w.device_ptr == nullptr && w.device == -1);
  // a thousand ranges inside one allocation: one attributes call, one range call
  {
    Allocations al;
    F.n.clear();
    for (int i = 0; i < 1000; i++) CHECK(al.check(ptr(A + uintptr_t(i)), 4096 - uint64_t(i), 0, "data") == 0);
    CHECK(F.n["hipPointerGetAttributes"] == 1 && F.n["hipMemGetAddressRange"] == 1 && al.nseen == 1);
    CHECK(al.check(ptr(A + 100), 3997, 0, "wire") == HDFS_CRC32C_EINVAL);  // a remembered allocation still has an end
    std::snprintf(want, sizeof(want), "wire: 3997 bytes at %p run past the end of their device allocation", ptr(A + 100));
    CHECK(err_is(want) && F.n["hipPointerGetAttributes"] == 1);
    CHECK(al.check(ptr(A + 100), UINT64_MAX, 0, "wire") == HDFS_CRC32C_EINVAL);
    CHECK(al.check(ptr(B), 1, 0, "data") == HDFS_CRC32C_EINVAL && al.nseen == 1);  // failures are not remembered
  }
  // 65 allocations: 64 are remembered, the 65th is asked about every time and still answered right
  {
    const uintptr_t C = 0x7300'0000'0000ull;
    for (uintptr_t i = 0; i < 65; i++) fake_block(C + i * 8192, 4096, 0);
    Allocations al;
    for (uintptr_t i = 0; i < 65; i++) CHECK(al.check(ptr(C + i * 8192 + 1), 4095, 0, "data") == 0);
    CHECK(al.nseen == 64);
    F.n.clear();
    CHECK(al.check(ptr(C + 63 * 8192), 4096, 0, "data") == 0 && F.n["hipPointerGetAttributes"] == 0);
    CHECK(al.check(ptr(C + 64 * 8192), 4096, 0, "data") == 0 && al.check(ptr(C + 64 * 8192 + 4095), 1, 0, "data") == 0);
    CHECK(F.n["hipPointerGetAttributes"] == 2 && F.n["hipMemGetAddressRange"] == 2 && al.nseen == 64);
    CHECK(al.check(ptr(C + 64 * 8192 + 1), 4096, 0, "data") == HDFS_CRC32C_EINVAL);
    CHECK(al.check(ptr(C + 64 * 8192 + 4096), 1, 0, "data") == HDFS_CRC32C_EINVAL);  // the gap behind it
    for (uintptr_t i = 0; i < 65; i++) F.blocks.erase(C + i * 8192);
  }
  F.blocks.erase(A);
  F.blocks.erase(B);
  F.blocks.erase(H);
}

// ---- a batch: no stream over another stream or over any data -----------------------------------------
using hdfs_wire::Span;  // companion_support.h's, through the using declaration of wire_batch_layout.h

// The nouns the libraries give the sweep: the wire side's defaults, and the read batches'.
const SpanNouns kNouns[2] = {SpanNouns{}, SpanNouns{"dst", "stream"}};

bool meet(const Span &a, const Span &b) { return a.lo < b.hi && b.lo < a.hi; }

// The verdict by looking at every pair, the sweep's yardstick.
bool scan_finds_overlap(const std::vector<Span> &v) {
  for (size_t i = 0; i < v.size(); i++)
    for (size_t j = i + 1; j < v.size(); j++)
      if ((v[i].wire || v[j].wire) && meet(v[i], v[j])) return true;
  return false;
}

// "entry A: <writer> overlaps the <writer|reader> of entry B" names spans of v that do overlap.
bool refusal_names_a_pair(const std::vector<Span> &v, const SpanNouns &nouns) {
  unsigned a = 0, b = 0;
  char first[8] = "", kind[8] = "";
  if (std::sscanf(last_error(), "entry %u: %7s overlaps the %7s of entry %u", &a, first, kind, &b) != 4) return false;
  if (std::strcmp(first, nouns.writer)) return false;
  const bool other_wire = !std::strcmp(kind, nouns.writer);
  if (!other_wire && std::strcmp(kind, nouns.reader)) return false;
  if (other_wire && a <= b) return false;  // the later entry is the one refused
  for (const Span &x : v)
    for (const Span &y : v)
      if (&x != &y && x.wire && x.k == a && y.wire == (other_wire ? 1u : 0u) && y.k == b && meet(x, y)) return true;
  return false;
}

// The sweep sorts its argument; the scan sees the caller's order.
int g_refused = 0, g_allowed = 0;
void overlaps_agree(const std::vector<Span> &v) {
  const bool bad = scan_finds_overlap(v);
  (bad ? g_refused : g_allowed)++;
  for (const SpanNouns &nouns : kNouns) {
    std::vector<Span> sorted = v;
    const int rc = hdfs_wire::check_overlaps(sorted, nullptr, nullptr, nouns);
    const std::string text = rc ? last_error() : "";
    // the written and the read ranges handed over apart, in the caller's order: the same verdict, the same text
    std::vector<Span> writers, readers;
    for (const Span &s : v) (s.wire ? writers : readers).push_back(s);
    Span sw{}, so{};
    const int rc2 = check_overlaps(writers, readers, &sw, &so, nouns);
    const bool same = rc2 == rc && (!rc || (text == last_error() && sw.wire && meet(sw, so)));
    if (same && rc == (bad ? HDFS_CRC32C_EINVAL : 0) && (!bad || refusal_names_a_pair(v, nouns))) continue;
    if (!same) std::printf("  apart: rc %d, text \"%s\"\n", rc2, rc2 ? last_error() : "");
    std::printf("  spans:");
    for (const Span &s : v)
      std::printf(" %s%u[%llu,%llu)", s.wire ? "w" : "d", s.k, (unsigned long long)s.lo, (unsigned long long)s.hi);
    std::printf("\n  rc %d, scan %d, text \"%s\"\n", rc, int(bad), rc ? last_error() : "");
    CHECK(!"check_overlaps agrees with the scan of every pair");
  }
}

// A wire-side text with the read batches' nouns.
std::string with_nouns(std::string text, const SpanNouns &nouns) {
  for (const char *old : {"wire", "data"}) {
    const std::string now = old[0] == 'w' ? nouns.writer : nouns.reader;
    for (size_t at = 0; (at = text.find(old, at)) != std::string::npos; at += now.size()) text.replace(at, 4, now);
  }
  return text;
}

void test_overlaps() {
  const uintptr_t B = 0x7400'0000'0000ull;
  auto one = [&](std::vector<Span> v, const char *text) {
    for (Span &s : v) s.lo += B, s.hi += B;
    overlaps_agree(v);
    int rc = hdfs_wire::check_overlaps(v);  // the defaults
    CHECK(text ? rc == HDFS_CRC32C_EINVAL && err_is(text) : rc == 0);
    for (const SpanNouns &nouns : kNouns) {  // the same entries whatever the ranges are called
      Span sw{}, so{};
      rc = hdfs_wire::check_overlaps(v, &sw, &so, nouns);
      CHECK(text ? rc == HDFS_CRC32C_EINVAL && err_is(with_nouns(text, nouns).c_str()) : rc == 0);
      CHECK(!text || (sw.wire && meet(sw, so)));  // the ranges at fault: a written one and what it overlaps
    }
  };
  one({}, nullptr);
  one({{0, 10, 0, 1}}, nullptr);
  one({{0, 10, 0, 1}, {10, 20, 1, 1}, {20, 30, 1, 0}, {30, 31, 0, 0}}, nullptr);  // touching: hi == lo
  one({{0, 10, 0, 0}, {5, 15, 1, 0}, {0, 15, 2, 0}, {20, 30, 0, 1}, {30, 40, 1, 1}}, nullptr);  // data over data
  one({{0, 10, 0, 1}, {9, 20, 1, 1}}, "entry 1: wire overlaps the wire of entry 0");
  one({{9, 20, 0, 1}, {0, 10, 1, 1}}, "entry 1: wire overlaps the wire of entry 0");
  one({{0, 10, 3, 1}, {9, 20, 3, 0}}, "entry 3: wire overlaps the data of entry 3");  // a write framed in place
  one({{0, 10, 0, 0}, {9, 20, 1, 1}}, "entry 1: wire overlaps the data of entry 0");
  // the same first byte: the wire range is sorted ahead of the data range, and refused either way
  one({{5, 6, 0, 0}, {5, 9, 1, 1}}, "entry 1: wire overlaps the data of entry 0");
  one({{5, 9, 0, 0}, {5, 6, 1, 1}}, "entry 1: wire overlaps the data of entry 0");
  one({{5, 9, 2, 1}, {5, 6, 1, 1}}, "entry 2: wire overlaps the wire of entry 1");
  one({{5, 9, 7, 0}, {5, 6, 7, 1}}, "entry 7: wire overlaps the data of entry 7");  // a read into its own stream
  // a long wire range swallows later spans that end long before it does
  one({{0, 100, 0, 1}, {100, 110, 1, 1}, {110, 120, 2, 0}}, nullptr);
  one({{0, 100, 0, 1}, {200, 210, 1, 1}, {220, 230, 2, 0}, {240, 250, 3, 1}, {90, 91, 4, 0}},
      "entry 0: wire overlaps the data of entry 4");
  one({{0, 100, 0, 1}, {200, 210, 1, 0}, {10, 12, 2, 0}, {20, 22, 3, 0}, {50, 51, 4, 1}},
      "entry 0: wire overlaps the data of entry 2");
  // ... and a long data range a later wire range, behind shorter data ranges
  one({{0, 100, 0, 0}, {10, 12, 1, 0}, {20, 22, 2, 0}, {99, 120, 3, 1}}, "entry 3: wire overlaps the data of entry 0");
  one({{0, 100, 0, 0}, {10, 12, 1, 0}, {20, 22, 2, 0}, {100, 120, 3, 1}}, nullptr);
  // every batch of up to 4 entries whose one range is [lo, hi) of 6 grid points, wire or data, or empty data
  // (which the front end leaves out, so the entry has no span)
  struct Choice {
    uint32_t lo, hi, wire;  // lo == hi: the empty one
  };
  std::vector<Choice> choices{{0, 0, 0}};
  for (uint32_t lo = 0; lo < 6; lo++)
    for (uint32_t hi = lo + 1; hi < 6; hi++)
      for (uint32_t wire = 0; wire < 2; wire++) choices.push_back({lo, hi, wire});
  CHECK(choices.size() == 31);
  g_refused = g_allowed = 0;
  std::vector<Span> v;
  for (size_t n = 1; n <= 4; n++) {
    size_t total = 1;
    for (size_t k = 0; k < n; k++) total *= choices.size();
    for (size_t code = 0; code < total; code++) {
      v.clear();
      size_t c = code;
      for (uint32_t k = 0; k < n; k++, c /= choices.size()) {
        const Choice &ch = choices[c % choices.size()];
        if (ch.lo != ch.hi) v.push_back(Span{B + 16 * ch.lo, B + 16 * ch.hi, k, ch.wire});
      }
      overlaps_agree(v);
    }
  }
  CHECK(g_refused > 100000 && g_allowed > 100000);
  // random batches of up to 32 entries (64 spans), fixed seed: streams laid out one behind another with gaps of
  // 0 to 3 bytes in a shuffled order, data anywhere in a region of its own, overlapping freely; then, in two
  // batches of three, one range is moved or stretched by a few bytes
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](uint64_t n) {
    seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
    return (seed >> 11) % n;
  };
  g_refused = g_allowed = 0;
  for (int round = 0; round < 4000; round++) {
    const uint32_t n = 1 + uint32_t(rnd(32));
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; k++) order[k] = k;
    for (uint32_t k = n; k > 1; k--) std::swap(order[k - 1], order[rnd(k)]);
    v.clear();
    uintptr_t at = B;
    for (uint32_t k : order) {
      const uintptr_t len = 1 + rnd(40);
      at += rnd(4);
      v.push_back(Span{at, at + len, k, 1u});
      at += len;
    }
    const uintptr_t D = at + 64;  // the data region
    for (uint32_t k = 0; k < n; k++)
      if (rnd(4)) {
        const uintptr_t lo = D + rnd(40 * n);
        v.push_back(Span{lo, lo + 1 + rnd(60), k, 0u});
      }
    if (round % 3) {
      Span &s = v[rnd(v.size())];
      switch (rnd(3)) {
        case 0: s.hi += 1 + rnd(8); break;
        case 1: s.lo -= 1 + rnd(8); break;
        default: {  // somewhere else altogether, streams and data alike
          const uintptr_t len = s.hi - s.lo;
          s.lo = B + rnd(D - B + 40 * n);
          s.hi = s.lo + len;
        }
      }
    }
    for (size_t k = v.size(); k > 1; k--) std::swap(v[k - 1], v[rnd(k)]);
    overlaps_agree(v);
  }
  CHECK(g_refused > 500 && g_allowed > 500);
}

// ---- the batch front end, on an entry struct of the public layout ---------------------------------------
struct TestEntry {
  const void *data;
  uint64_t len;
  int64_t offset_in_block, seqno;
  int32_t finish, reserved;
  void *wire;
  uint64_t wire_cap;
  uint64_t wire_len, npkts, first_pkt;  // out
};
struct TestTotals {
  uint64_t npkts, nchunks, wire_bytes, table_entries;
};

// A library's layout_batch with a limit of its own: at most max_packets, judged behind the walk.
int test_layout_batch(TestEntry *w, size_t n, uint64_t max_packets, hdfs_wire::Batch &B) {
  hdfs_wire::Counts c;
  int rc = hdfs_wire::count_batch(w, n, 5, 2, HDFS_CRC32C_CSUM_CRC32C, c);
  if (rc || (rc = hdfs_wire::layout_entries(w, n, 2, HDFS_CRC32C_CSUM_CRC32C, B))) return rc;
  CHECK(B.npkts == c.packets && B.nchunks == c.chunks);  // the closed forms count what the walk finds
  return B.npkts > max_packets ? fail(HDFS_CRC32C_EINVAL, "too many packets") : HDFS_CRC32C_OK;
}

void test_batch_front_end() {
  using namespace hdfs_wire;
  const uintptr_t A = 0x7500'0000'0000ull, W = 0x7600'0000'0000ull, H = 0x7700'0000'0000ull;
  auto ptr = [](uintptr_t a) { return reinterpret_cast<void *>(a); };
  fake_block(A, 1 << 20, 0);
  fake_block(W, 1 << 20, 0);
  fake_block(H, 4096, 0, true);
  // four writes: a short head chunk and two packets; an empty one with finish; an empty one without (no
  // packet); 65 537 bytes on the grid with finish
  auto fresh = [&] {
    std::vector<TestEntry> w(4);
    std::memset(w.data(), 0, w.size() * sizeof(TestEntry));
    w[0] = TestEntry{ptr(A), 65536, 1, 10, 0, 0, ptr(W), 70000, 9, 9, 9};
    w[1] = TestEntry{nullptr, 0, 0, 20, 1, 0, ptr(W + 100000), 100, 9, 9, 9};
    w[2] = TestEntry{nullptr, 0, 5, 30, 0, 0, ptr(W + 100200), 0, 9, 9, 9};
    w[3] = TestEntry{ptr(A + 200000), 65537, 512, 40, 1, 0, ptr(W + 200000), 70000, 9, 9, 9};
    return w;
  };
  std::vector<TestEntry> w = fresh();
  const uint64_t hb = hdfs_crc32c::outpkt::out_header_bytes(2);
  // the list and the arguments
  Counts c;
  CHECK(count_batch(w.data(), 6, 5, 2, 2, c) == HDFS_CRC32C_EINVAL && err_is("6 writes, at most 5 in one call"));
  CHECK(w[0].npkts == 9);  // nothing written yet
  CHECK(count_batch<TestEntry>(nullptr, 1, 5, 2, 2, c) == HDFS_CRC32C_EINVAL && err_is("null writes"));
  CHECK(count_batch<TestEntry>(nullptr, 0, 5, 2, 2, c) == 0 && c.chunks == 0 && c.packets == 0);
  w[2].offset_in_block = -1;
  CHECK(count_batch(w.data(), 4, 5, 2, 2, c) == HDFS_CRC32C_EINVAL && err_is("entry 2: negative block offset"));
  for (const TestEntry &e : w) CHECK(e.wire_len == 0 && e.npkts == 0 && e.first_pkt == 0);  // zeroed ahead of any refusal
  CHECK(count_batch(w.data(), 4, 5, 3, 2, c) == HDFS_CRC32C_EINVAL && err_is("entry 0: proto must be 1 or 2"));
  // the counts in closed form: 511 + 65025 bytes are 1 + 128 chunks in 1 + 1 packets; finish alone is a packet;
  // 65537 bytes on the grid are 129 chunks in 2 packets, and finish
  w = fresh();
  c = Counts{};
  CHECK(count_batch(w.data(), 4, 5, 2, 2, c) == 0 && c.chunks == 129 + 0 + 0 + 129 && c.packets == 2 + 1 + 0 + 3);
  // the walk fills every entry's out fields before the library judges the totals
  {
    Batch B;
    CHECK(test_layout_batch(w.data(), 4, 5, B) == HDFS_CRC32C_EINVAL && err_is("too many packets"));
    CHECK(w[0].npkts == 2 && w[1].npkts == 1 && w[2].npkts == 0 && w[3].npkts == 3);
    CHECK(w[0].first_pkt == 0 && w[1].first_pkt == 2 && w[2].first_pkt == 3 && w[3].first_pkt == 3);
    CHECK(w[0].wire_len == 65536 + 2 * hb + 4 * 129 && w[1].wire_len == hb && w[2].wire_len == 0);
    CHECK(B.npkts == 6 && B.nchunks == 258 && B.entries == 3 && B.wire_bytes == w[0].wire_len + hb + w[3].wire_len);
    // the _layout entry point: the totals are written even when the layout is refused
    TestTotals t;
    std::memset(&t, 0xEE, sizeof(t));
    std::vector<TestEntry> w2 = fresh();
    CHECK(layout_totals(&t, [&](Batch &b) { return test_layout_batch(w2.data(), 4, 5, b); }) == HDFS_CRC32C_EINVAL);
    CHECK(t.npkts == 6 && t.nchunks == 258 && t.wire_bytes == B.wire_bytes && t.table_entries == 3);
    CHECK(layout_totals(&t, [&](Batch &b) { return test_layout_batch(w2.data(), 4, 6, b); }) == 0 && t.npkts == 6);
    CHECK(layout_totals(static_cast<TestTotals *>(nullptr), [&](Batch &) { return 0; }) == HDFS_CRC32C_EINVAL);
    CHECK(err_is("null out"));
  }
  Batch B;
  CHECK(test_layout_batch(w.data(), 4, 6, B) == 0);
  // the records: every write's at its first_pkt
  {
    std::vector<hdfs_crc32c_out_packet> pk(6);
    std::memset(pk.data(), 0xEE, pk.size() * sizeof(pk[0]));
    fill_batch_records(w.data(), B, pk.data());
    CHECK(pk[0].seqno == 10 && pk[1].seqno == 11 && pk[2].seqno == 20 && pk[3].seqno == 40 && pk[5].seqno == 42);
    CHECK(pk[0].data_len == 511 && pk[2].last == 1 && pk[2].data_len == 0 && pk[5].last == 1 && pk[4].hdr_off);
  }
  // a call that has stream buffers: all or none
  CHECK(count_wires(w.data(), 4) == 4 && count_wires(w.data(), 0) == 0);
  CHECK(check_entries(w.data(), 4, 4, B, nullptr, 0) == 0);
  w[2].wire = w[3].wire = nullptr;
  CHECK(count_wires(w.data(), 4) == 2 && check_entries(w.data(), 4, 2, B, nullptr, 0) == HDFS_CRC32C_EINVAL);
  CHECK(err_is("entry 2: wire is NULL, entry 0's is not (every wire NULL is a size query)"));  // the first that differs
  w = fresh();
  w[0].wire = w[1].wire = nullptr;
  CHECK(test_layout_batch(w.data(), 4, 6, B = Batch{}) == 0 && count_wires(w.data(), 4) == 2);
  CHECK(check_entries(w.data(), 4, 2, B, nullptr, 0) == HDFS_CRC32C_EINVAL);
  CHECK(err_is("entry 2: wire is set, entry 0's is not (every wire NULL is a size query)"));
  // every entry's own room, in entry order and data first
  w = fresh();
  CHECK(test_layout_batch(w.data(), 4, 6, B = Batch{}) == 0);
  char want[256];
  w[3].data = nullptr;
  w[1].wire_cap = hb - 1;
  std::snprintf(want, sizeof(want), "entry 1: %llu stream bytes, room for %llu", (unsigned long long)hb, (unsigned long long)hb - 1);
  CHECK(check_entries(w.data(), 4, 4, B, nullptr, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  w[1].wire_cap = hb;
  CHECK(check_entries(w.data(), 4, 4, B, nullptr, 0) == HDFS_CRC32C_EINVAL && err_is("entry 3: null data with 65537 bytes"));
  w[3].data = ptr(A + 200000);
  w[3].wire_cap = w[3].wire_len - 1;
  std::snprintf(want, sizeof(want), "entry 3: %llu stream bytes, room for %llu", (unsigned long long)w[3].wire_len,
                (unsigned long long)w[3].wire_len - 1);
  CHECK(check_entries(w.data(), 4, 4, B, nullptr, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  w[3].wire_cap = w[3].wire_len;
  std::vector<hdfs_crc32c_out_packet> pk(6);
  CHECK(check_entries(w.data(), 4, 4, B, pk.data(), 6) == 0 && check_entries(w.data(), 4, 4, B, nullptr, 0) == 0);
  CHECK(check_entries(w.data(), 4, 4, B, pk.data(), 5) == HDFS_CRC32C_EINVAL);
  CHECK(err_is("entry 3: its records end at 6 of 6, room for 5"));
  CHECK(check_entries(w.data(), 4, 4, B, pk.data(), 1) == HDFS_CRC32C_EINVAL);
  CHECK(err_is("entry 0: its records end at 2 of 6, room for 1"));
  // where the buffers lie: two allocations, asked about once each; the entries without bytes are not asked about
  F.n.clear();
  CHECK(check_batch_places(w.data(), 4, 0) == 0);
  CHECK(F.n["hipPointerGetAttributes"] == 2 && F.n["hipMemGetAddressRange"] == 2);
  w[2].wire = ptr(uintptr_t(0x10));  // no stream bytes: any address
  CHECK(check_batch_places(w.data(), 4, 0) == 0);
  w[3].data = ptr(H);
  std::snprintf(want, sizeof(want), "entry 3: data: %p is not device memory", ptr(H));
  CHECK(check_batch_places(w.data(), 4, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  w[3].data = ptr(A + (1 << 20) - 65536);
  std::snprintf(want, sizeof(want), "entry 3: data: 65537 bytes at %p run past the end of their device allocation", w[3].data);
  CHECK(check_batch_places(w.data(), 4, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  w[3].data = ptr(A + 200000);
  w[1].wire = ptr(W + (1 << 20) - (hb - 1));
  std::snprintf(want, sizeof(want), "entry 1: wire: %llu bytes at %p run past the end of their device allocation",
                (unsigned long long)hb, w[1].wire);
  CHECK(check_batch_places(w.data(), 4, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  w[1].wire = ptr(W + w[0].wire_len - 1);
  CHECK(check_batch_places(w.data(), 4, 0) == HDFS_CRC32C_EINVAL && err_is("entry 1: wire overlaps the wire of entry 0"));
  w[1].wire = ptr(W + w[0].wire_len);  // touching
  CHECK(check_batch_places(w.data(), 4, 0) == 0);
  w[3].wire = ptr(A + 65535);
  CHECK(check_batch_places(w.data(), 4, 0) == HDFS_CRC32C_EINVAL && err_is("entry 3: wire overlaps the data of entry 0"));
  w[3].wire = ptr(A + 65536);
  CHECK(check_batch_places(w.data(), 4, 0) == 0);  // behind entry 0's data, ahead of its own
  w[3].wire = ptr(W + 200000);
  w[3].data = w[0].data;  // two writes of the same bytes
  CHECK(check_batch_places(w.data(), 4, 0) == 0);

  // a gather write: the fragments and the stream (companion_support.h's check_places)
  hdfs_crc32c_iovec iov[4] = {{ptr(A), 100}, {nullptr, 0}, {ptr(H), 0}, {ptr(A + 50), 100}};
  F.n.clear();
  CHECK(check_places(iov, 4, ptr(W), 300, 0) == 0 && F.n["hipPointerGetAttributes"] == 2);
  CHECK(check_places(iov, 4, ptr(A + 150), 300, 0) == 0);  // touching the last fragment
  CHECK(check_places(iov, 4, ptr(A + 149), 300, 0) == HDFS_CRC32C_EINVAL && err_is("fragment 3 and wire overlap"));
  CHECK(check_places(iov, 4, ptr(A + 99), 1, 0) == HDFS_CRC32C_EINVAL && err_is("fragment 0 and wire overlap"));
  CHECK(check_places(iov, 4, ptr(W + (1 << 20) - 299), 300, 0) == HDFS_CRC32C_EINVAL);
  std::snprintf(want, sizeof(want), "wire: 300 bytes at %p run past the end of their device allocation", ptr(W + (1 << 20) - 299));
  CHECK(err_is(want));
  iov[2].len = 8;
  std::snprintf(want, sizeof(want), "fragment 2: data: %p is not device memory", ptr(H));
  CHECK(check_places(iov, 4, ptr(W), 300, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  F.blocks.erase(A);
  F.blocks.erase(W);
  F.blocks.erase(H);
}

// ---- the arguments and the chunk grid ---------------------------------------------------------------
void test_args_and_grid() {
  using namespace hdfs_wire;
  CHECK(packet_args_ok(1, 0, 0) && packet_args_ok(2, 2, INT64_MAX) && packet_args_ok(2, 1, 0));
  CHECK(!packet_args_ok(0, 2, 0) && err_is("proto must be 1 or 2"));
  CHECK(!packet_args_ok(3, 2, 0) && err_is("proto must be 1 or 2"));
  CHECK(!packet_args_ok(2, 3, 0) && err_is("bad checksum type 3"));
  CHECK(!packet_args_ok(2, -1, 0) && err_is("bad checksum type -1"));
  CHECK(!packet_args_ok(2, 2, -1) && err_is("negative block offset"));
  CHECK(!packet_args_ok(7, 9, -1) && err_is("proto must be 1 or 2"));  // the first complaint wins
  CHECK(args_ok(2, 2, 0, uint64_t(1) << 40) && !args_ok(2, 2, 0, (uint64_t(1) << 40) + 1));
  CHECK(err_is("more than 1 TiB in one write") && !args_ok(2, 2, -1, ~uint64_t(0)) && err_is("negative block offset"));

  const uint8_t *data = reinterpret_cast<const uint8_t *>(uintptr_t(0x10000));
  uint32_t *crc = reinterpret_cast<uint32_t *>(uintptr_t(0x90000));
  for (uint64_t len : {0, 1, 511, 512, 513})
    for (int64_t off : {0, 1, 511})
      for (int ctype : {HDFS_CRC32C_CSUM_NULL, HDFS_CRC32C_CSUM_CRC32, HDFS_CRC32C_CSUM_CRC32C}) {
        Layout L;
        CHECK(build_layout(len, off, 0, 2, ctype, false, L) == 0);
        Write w = L.w;
        w.data = data;
        // the grid, worked out here: the bytes up to the next multiple of 512 of the block offset, then the rest
        const uint64_t n0 = len && off % 512 ? std::min<uint64_t>(len, 512 - uint64_t(off % 512)) : 0;
        CHECK(w.n0 == n0);
        hdfs_crc32c_segment s[3];
        std::memset(s, 0xEE, sizeof(s));
        const size_t ns = grid_segments(w, crc, ctype, s);
        if (ctype == HDFS_CRC32C_CSUM_NULL || !len) {
          CHECK(ns == 0);
          continue;
        }
        const uint32_t flags = HDFS_CRC32C_SEG_BE | (ctype == HDFS_CRC32C_CSUM_CRC32 ? HDFS_CRC32C_SEG_CRC32 : 0u);
        CHECK(ns == (n0 ? 1u : 0u) + (len > n0 ? 1u : 0u));
        size_t i = 0;
        uint64_t chunks = 0;
        if (n0) {  // the head segment; alone when len - n0 == 0
          CHECK(s[i].data == data && s[i].len == n0 && s[i].crcs == crc);
          chunks += 1;
          i++;
        }
        if (len > n0) {
          CHECK(s[i].data == data + n0 && s[i].len == len - n0 && s[i].crcs == crc + (n0 ? 1 : 0));
          chunks += (len - n0 + 511) / 512;
          i++;
        }
        CHECK(i == ns && chunks == L.nchunks);
        for (size_t k = 0; k < ns; k++)
          CHECK(s[k].chunk_size == 512 && s[k].flags == flags && s[k].crc_init == 0 && s[k].reserved == 0 &&
                s[k].bitmap == nullptr);
        uint8_t untouched[sizeof(s[0])];
        std::memset(untouched, 0xEE, sizeof(untouched));
        CHECK(!std::memcmp(&s[2], untouched, sizeof(untouched)));
      }
}

// ---- the end of a call, and the timed frame run ---------------------------------------------------------
void test_tail_and_run() {
  hipStream_t st = nullptr;
  size_t at = F.log.size();
  CHECK(sync_and_report(st, hipSuccess, 0, kPlan, "gather write") == 0 && names_since(at) == "hipStreamSynchronize plan_destroy");
  at = F.log.size();
  CHECK(sync_and_report(st, hipSuccess, 0, nullptr, "block digests") == 0 && names_since(at) == "hipStreamSynchronize");
  // an error so far: synchronised all the same, the plan destroyed once
  at = F.log.size();
  CHECK(sync_and_report(st, hipErrorOutOfMemory, 0, kPlan, "wire stream") == HDFS_CRC32C_EHIP);
  CHECK(err_is("wire stream: fake: out of memory") && names_since(at) == "hipStreamSynchronize plan_destroy");
  // the first error is the one reported, the synchronise's own only when there was none
  F.fail_sync = 1;
  CHECK(sync_and_report(st, hipErrorOutOfMemory, 0, nullptr, "w") == HDFS_CRC32C_EHIP && err_is("w: fake: out of memory"));
  F.fail_sync = 1;
  CHECK(sync_and_report(st, hipSuccess, 0, nullptr, "w") == HDFS_CRC32C_EHIP && err_is("w: fake: launch failure"));
  F.sticky = hipSuccess;  // a failed synchronise is the caller's to clear, as it was
  // the engine's rc wins over the HIP error, and its text stays
  fail(-5, "compute plan: engine said no");
  at = F.log.size();
  CHECK(sync_and_report(st, hipErrorOutOfMemory, -5, kPlan, "wire batch") == -5);
  CHECK(err_is("compute plan: engine said no") && names_since(at) == "hipStreamSynchronize plan_destroy");

  using hdfs_wire::timed_frame_run;
  hipEvent_t ev[2] = {nullptr, nullptr};
  double ms = -1;
  int launches = 0;
  auto launch = [&] {
    F.called("launch");
    launches++;
    return F.fail_launch && launches == F.fail_launch ? hipErrorLaunchFailure : hipSuccess;
  };
  // the plain call: execute, one launch, synchronise, destroy; no event call
  at = F.log.size();
  CHECK(timed_frame_run(st, hipSuccess, kPlan, ev, 0, nullptr, "wire stream", launch) == 0);
  CHECK(names_since(at) == "plan_execute launch hipStreamSynchronize plan_destroy" && ms == -1);
  at = F.log.size();
  CHECK(timed_frame_run(st, hipSuccess, nullptr, ev, 0, nullptr, "wire stream", launch) == 0);
  CHECK(names_since(at) == "launch hipStreamSynchronize");
  // the timing call
  at = F.log.size();
  CHECK(timed_frame_run(st, hipSuccess, kPlan, ev, 3, &ms, "wire batch", launch) == 0 && ms == 2.0);
  CHECK(names_since(at) == "plan_execute launch hipEventRecord launch launch launch hipEventRecord "
                           "hipStreamSynchronize plan_destroy hipEventElapsedTime");
  // the caller's own enqueue failed: nothing runs, still synchronised, the plan destroyed
  at = F.log.size();
  CHECK(timed_frame_run(st, hipErrorOutOfMemory, kPlan, ev, 2, &ms, "wire batch", launch) == HDFS_CRC32C_EHIP);
  CHECK(err_is("wire batch: fake: out of memory") && names_since(at) == "hipStreamSynchronize plan_destroy");
  // the plan fails: no launch, the engine's rc and text
  F.exec_rc = -4;
  F.engine_text = "bad segment";
  at = F.log.size();
  CHECK(timed_frame_run(st, hipSuccess, kPlan, ev, 2, &ms, "wire stream", launch) == -4);
  CHECK(err_is("compute plan: bad segment") && names_since(at) == "plan_execute hipStreamSynchronize plan_destroy");
  F.exec_rc = 0;
  // a launch fails among the timed ones: the rest is skipped, no time is read
  launches = 0;
  F.fail_launch = 2;
  at = F.log.size();
  CHECK(timed_frame_run(st, hipSuccess, kPlan, ev, 3, &ms, "wire stream", launch) == HDFS_CRC32C_EHIP);
  CHECK(err_is("wire stream: fake: launch failure") &&
        names_since(at) == "plan_execute launch hipEventRecord launch hipStreamSynchronize plan_destroy");
  F.fail_launch = 0;
}


// ---- the read side: the probed run ---------------------------------------------------------------
void test_probed_run() {
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  TablePair tab;
  CHECK(tab.reserve(4096, kTableFloor) == 0);
  const uint8_t *pin = tab.pin.as<uint8_t>(), *dv = tab.dev.as<uint8_t>();
  int launches = 0;
  auto launch = [&] {
    F.called("launches");
    launches++;
    return F.fail_launch && launches == F.fail_launch ? hipErrorLaunchFailure : hipSuccess;
  };
  auto run = [&](int iters, double *ms) {
    launches = 0;
    F.copies.clear();
    return probed_run(st, tab, 64, 160, 1024, 4096, ev, iters, ms, "read batch", launch);
  };
  // the plain call: the upload, one round, the copy back, the synchronise; no event call
  size_t at = F.log.size();
  CHECK(run(0, nullptr) == 0 && launches == 1);
  CHECK(names_since(at) == "hipMemcpyAsync launches hipMemcpyAsync hipStreamSynchronize");
  CHECK(F.copies.size() == 2 && F.copies[0].dst == dv + 64 && F.copies[0].src == pin + 64 && F.copies[0].n == 160 &&
        F.copies[0].kind == hipMemcpyHostToDevice);
  CHECK(F.copies[1].dst == pin + 1024 && F.copies[1].src == dv + 1024 && F.copies[1].n == 4096 - 1024 &&
        F.copies[1].kind == hipMemcpyDeviceToHost);
  // the timing call: the copy back stays between the first round and the first event
  for (int iters : {1, 3}) {
    double ms = -1;
    at = F.log.size();
    CHECK(run(iters, &ms) == 0 && launches == 1 + iters && ms == 6.0 / iters && F.copies.size() == 2);
    std::string want = "hipMemcpyAsync launches hipMemcpyAsync hipEventRecord";
    for (int i = 0; i < iters; i++) want += " launches";
    CHECK(names_since(at) == want + " hipEventRecord hipStreamSynchronize hipEventElapsedTime");
  }
  // a failing upload: no launch, still synchronised
  double ms = 0;
  F.fail_async = 1;
  at = F.log.size();
  CHECK(run(2, &ms) == HDFS_CRC32C_EHIP && err_is("read batch: fake: out of memory") && launches == 0 && ms == 0);
  CHECK(names_since(at) == "hipMemcpyAsync hipStreamSynchronize");
  // ... a failing copy back: no event
  F.fail_async = 2;
  at = F.log.size();
  CHECK(run(2, &ms) == HDFS_CRC32C_EHIP && err_is("read batch: fake: out of memory") && launches == 1 && ms == 0);
  CHECK(names_since(at) == "hipMemcpyAsync launches hipMemcpyAsync hipStreamSynchronize");
  // a launch failing at the first call: nothing comes back
  F.fail_launch = 1;
  at = F.log.size();
  CHECK(run(3, &ms) == HDFS_CRC32C_EHIP && err_is("read batch: fake: launch failure") && ms == 0);
  CHECK(names_since(at) == "hipMemcpyAsync launches hipStreamSynchronize");
  // ... and at the second round of the timed loop: no second event, no time read
  F.fail_launch = 3;
  at = F.log.size();
  CHECK(run(3, &ms) == HDFS_CRC32C_EHIP && err_is("read batch: fake: launch failure") && ms == 0);
  CHECK(names_since(at) ==
        "hipMemcpyAsync launches hipMemcpyAsync hipEventRecord launches launches hipStreamSynchronize");
  F.fail_launch = 0;
  // a failing synchronise after a clean queue, plain and timed
  for (int iters : {0, 2}) {
    F.fail_sync = 1;
    at = F.log.size();
    CHECK(run(iters, iters ? &ms : nullptr) == HDFS_CRC32C_EHIP && err_is("read batch: fake: launch failure") && ms == 0);
    CHECK(names_since(at).find("hipEventElapsedTime") == std::string::npos && F.log.back() == "hipStreamSynchronize@0");
  }
  F.sticky = hipSuccess;  // the fake's record of the failures above; the run clears nothing, as before
  // a timing call's own arguments, before any runtime call
  at = F.log.size();
  CHECK(timing_args_ok(0, &ms) == HDFS_CRC32C_EINVAL && err_is("iters >= 1 and ms_per_iter are needed"));
  CHECK(timing_args_ok(-1, &ms) == HDFS_CRC32C_EINVAL && timing_args_ok(1, nullptr) == HDFS_CRC32C_EINVAL);
  CHECK(err_is("iters >= 1 and ms_per_iter are needed") && timing_args_ok(1, &ms) == 0 && F.log.size() == at);
  tab.release();
}

// ---- the read side: the entries' outcomes ------------------------------------------------------------
void test_outcomes() {
  {
    Outcomes o;
    o.note(0);
    o.note(3);
    o.note(fail(-2, "a"));
    o.note(fail(-5, "b"));
    o.note(1);
    fail(-9, "something later");
    CHECK(o.result() == -2 && err_is("a"));
  }
  {
    Outcomes o;
    for (int r : {0, 4, 0, 2}) o.note(r);
    fail(-9, "left alone");
    CHECK(o.result() == 4 && err_is("left alone"));
  }
  {
    Outcomes o;
    for (int i = 0; i < 5; i++) o.note(0);
    CHECK(o.result() == 0 && Outcomes{}.result() == 0);
  }
  // slot s of entry b: no slot, or a descriptor that names b back; entry_of is not asked about anything else
  const uint32_t entry[3] = {5, 6, 7}, none = 0xFFFFFFFFu;
  int asked = 0;
  auto of = [&](uint32_t s) { return asked++, entry[s]; };
  CHECK(slot_adds_up(none, none, 3, 6, of) && asked == 0);
  CHECK(slot_adds_up(1, none, 3, 6, of) && !slot_adds_up(1, none, 3, 5, of) && asked == 2);
  CHECK(!slot_adds_up(3, none, 3, 6, of) && !slot_adds_up(1, none, 1, 6, of) && !slot_adds_up(none - 1, none, 3, 6, of));
  CHECK(asked == 2 && tables_fail(1023) == HDFS_CRC32C_EHIP);
  CHECK(err_is("internal: the probe's tables do not add up at entry 1023"));
}

// ---- the read side: the main library's read with unlimited record room ------------------------------
void test_read_unlimited() {
  std::vector<hdfs_crc32c_packet> recs;
  const void *stream = reinterpret_cast<const void *>(uintptr_t(0x7800'0000'0000ull));
  const hdfs_crc32c_iovec iov[2] = {{nullptr, 0}, {nullptr, 0}};
  size_t np = 0;
  uint64_t used = 0, got = 0;
  auto read = [&](uint64_t len, hdfs_crc32c_packet *own, size_t own_room) {
    F.reads.clear();
    np = used = got = 0;
    return read_unlimited(recs, stream, len, 2, 512, 2, 11, 22, iov, 2, own, own_room, &np, &used, &got);
  };
  // 10 000 records in a stream that could hold 20 002: 4 096 do not do, 16 times as many would, cut to the most
  F.read_records = 10000;
  CHECK(read(25 * 20000, nullptr, 0) == 0 && np == 10000 && used == 25 * 20000 && got == 77);
  CHECK(F.reads.size() == 2 && F.reads[0].room == 4096 && F.reads[1].room == 20002 && recs.size() == 20002);
  CHECK(F.reads[1].pkts == recs.data() && recs[9999].offset_in_block == 10999);
  for (const Fake::Read &r : F.reads)
    CHECK(r.stream == stream && r.len == 25 * 20000 && r.client_offset == 11 && r.read_len == 22 && r.iov == iov &&
          r.iovcnt == 2);
  // ... that could hold 200 002: 65 536 are enough
  CHECK(read(25 * 200000, nullptr, 0) == 0 && np == 10000);
  CHECK(F.reads.size() == 2 && F.reads[0].room == 4096 && F.reads[1].room == 65536);
  // it ends when the records did not fill the room, and when the room is the most the stream can hold
  F.read_records = 4095;
  CHECK(read(25 * 200000, nullptr, 0) == 0 && np == 4095 && F.reads.size() == 1 && F.reads[0].room == 4096);
  F.read_records = 100;
  CHECK(read(100, nullptr, 0) == 0 && np == 6 && F.reads.size() == 1 && F.reads[0].room == 6);  // 100 / 25 + 2
  F.read_records = 70000;
  CHECK(read(25 * 69998, nullptr, 0) == 0 && np == 70000 && F.reads.size() == 3 && F.reads[2].room == 70000);
  // a packet error is an answer; an engine failure stops it at once
  F.read_records = 10000;
  F.read_rc = 7;
  CHECK(read(25 * 20000, nullptr, 0) == 7 && np == 10000 && F.reads.size() == 2);
  F.read_rc = -5;
  CHECK(read(25 * 20000, nullptr, 0) == -5 && F.reads.size() == 1 && np == 0);
  F.read_rc = 0;
  // with the caller's record array: one call, with the caller's room, however many records there are
  std::vector<hdfs_crc32c_packet> pkts(4 * 8);
  const size_t b = 3, max_pkts = 8;
  CHECK(read(25 * 20000, pkts.data() + b * max_pkts, max_pkts) == 0 && np == 8 && F.reads.size() == 1);
  CHECK(F.reads[0].pkts == pkts.data() + 24 && F.reads[0].room == 8 && pkts[31].offset_in_block == 1007);
  F.read_records = 0;
}

// ---- the read side: the main library's walk in pieces -------------------------------------------------
void test_walk_pieces() {
  std::vector<hdfs_crc32c_packet> recs;
  const uint8_t *s = reinterpret_cast<const uint8_t *>(uintptr_t(0x7900'0000'0000ull));
  struct Seen {
    uint64_t at, stream_off;
  };
  std::vector<Seen> seen;
  auto walk = [&](std::vector<Fake::Piece> pieces, uint64_t len) {
    F.pieces = pieces;
    F.parses.clear();
    seen.clear();
    return walk_pieces(recs, 4, s, len, 9, 2, 512, 2,
                       [&](const hdfs_crc32c_packet &k, uint64_t at) { seen.push_back(Seen{at, k.stream_off}); });
  };
  // two full pieces, then the empty last packet: every piece starts where the one before stopped
  Walk w = walk({{0, 4, 400, false}, {0, 4, 400, false}, {0, 2, 150, true}}, 1000);
  CHECK(w.rc == 0 && w.pos == 950 && w.npkts == 10 && w.payload == 90 && w.offset_in_block == 4096 + 1000);
  CHECK(F.parses.size() == 3 && F.parses[1].stream == s + 400 && F.parses[1].len == 600 && F.parses[2].stream == s + 800);
  CHECK(F.parses[0].room == 4 && recs.size() == 4 && seen.size() == 10 && seen[4].at == 400 && seen[4].stream_off == 0 &&
        seen[9].at == 800 && seen[9].stream_off == 100);
  // the empty last packet at the end of a full piece: no further call
  w = walk({{0, 4, 400, true}, {0, 1, 1, false}}, 1000);
  CHECK(w.rc == 0 && w.pos == 400 && w.npkts == 4 && w.payload == 30 && F.parses.size() == 1);
  // a piece shorter than its room (an incomplete packet behind it)
  w = walk({{0, 4, 400, false}, {0, 3, 300, false}, {0, 1, 1, false}}, 1000);
  CHECK(w.rc == 0 && w.pos == 700 && w.npkts == 7 && w.payload == 70 && F.parses.size() == 2);
  // a framing error: the packet that raises it is counted, not handed on, and the walk stops
  w = walk({{0, 4, 400, false}, {3, 4, 380, false}, {0, 1, 1, false}}, 1000);
  CHECK(w.rc == 3 && w.pos == 780 && w.npkts == 8 && w.payload == 70 && seen.size() == 7 && F.parses.size() == 2);
  // an engine failure: its rc, its text behind the entry and the call; what was walked stays
  F.engine_text = "no memory";
  w = walk({{0, 4, 400, false}, {-4, 0, 0, false}}, 1000);
  CHECK(w.rc == -4 && err_is("entry 9: parse_packets: no memory") && w.npkts == 4 && w.pos == 400 && w.payload == 40);
  CHECK(w.offset_in_block == 4096 + 1000);
  // a full piece that used no byte ends the walk; the stream's end does; an empty stream is not walked
  w = walk({{0, 4, 0, false}, {0, 1, 1, false}}, 1000);
  CHECK(w.rc == 0 && w.pos == 0 && w.npkts == 4 && F.parses.size() == 1);
  w = walk({{0, 4, 400, false}, {0, 4, 400, false}}, 800);
  CHECK(w.rc == 0 && w.pos == 800 && w.npkts == 8 && F.parses.size() == 2);
  w = walk({}, 0);
  CHECK(w.rc == 0 && w.pos == 0 && w.npkts == 0 && w.payload == 0 && w.offset_in_block == 0 && F.parses.empty());
  CHECK(kPieceRecords == 65536);
}

// ---- the read side: the scratch of a library that runs the fused round -----------------------------------
struct MoreScratch : ReadScratch<FusedState> {  // as the relay library builds its own
  DeviceBuffer more;
  int reserve(int to, size_t tab_bytes) {
    return ReadScratch::reserve(to, tab_bytes, [this] { more.release(); });
  }
};

void test_read_scratch() {
  const size_t live = F.blocks.size();
  ReadScratch<FusedState> s;
  F.cur = 0;
  g_prepares = 0;
  size_t at = F.log.size();
  CHECK(s.reserve(0, 100) == 0 && g_prepares == 1 && s.dev == 0 && s.fused.ready && s.tab.dev.cap == kTableFloor);
  CHECK(names_since(at) == "hipStreamCreate hipMalloc hipMemcpy hipDeviceGetAttribute prepare hipMalloc hipHostMalloc");
  at = F.log.size();
  CHECK(s.reserve(0, 16384) == 0 && s.reserve(0, 0) == 0 && F.log.size() == at && g_prepares == 1);  // a warm call
  // the engine moved to device 2: everything released on device 0, then built again
  F.cur = 2;
  at = F.log.size();
  CHECK(s.reserve(2, 100) == 0 && g_prepares == 2 && s.fused.ready && F.wrong_device_frees == 0);
  std::string got;
  for (size_t i = at; i < F.log.size(); i++) got += F.log[i] + " ";
  CHECK(got == "hipGetDevice@2 hipSetDevice@0 hipStreamSynchronize@0 hipFree@0 hipFree@0 hipHostFree@0 "
               "hipStreamDestroy@0 hipSetDevice@2 hipStreamCreate@2 hipMalloc@2 hipMemcpy@2 hipDeviceGetAttribute@2 "
               "prepare@2 hipMalloc@2 hipHostMalloc@2 ");
  // a failing prepare: EHIP, the text, bound but not ready; the next call prepares again
  F.cur = 1;
  g_prepare_rc = hipErrorLaunchFailure;
  CHECK(s.reserve(1, 100) == HDFS_CRC32C_EHIP && err_is("tables: fake: launch failure") && !s.fused.ready && s.dev == 1);
  CHECK(!s.tab.dev.p && F.wrong_device_frees == 0);
  g_prepare_rc = hipSuccess;
  at = F.log.size();
  CHECK(s.reserve(1, 100) == 0 && s.fused.ready);
  CHECK(names_since(at) == "hipMemcpy hipDeviceGetAttribute prepare hipMalloc hipHostMalloc");
  s.unbind([&] {
    s.fused.release();
    s.tab.release();
  });
  // a library's further buffers go with the rest, behind them
  MoreScratch m;
  F.cur = 0;
  CHECK(m.reserve(0, 100) == 0 && m.more.reserve(10, 0) == 0);
  F.cur = 2;
  at = F.log.size();
  CHECK(m.reserve(2, 100) == 0 && !m.more.p && F.wrong_device_frees == 0);
  got.clear();
  for (size_t i = at; i < F.log.size(); i++) got += F.log[i] + " ";
  CHECK(got.rfind("hipGetDevice@2 hipSetDevice@0 hipStreamSynchronize@0 hipFree@0 hipFree@0 hipHostFree@0 hipFree@0 "
                  "hipStreamDestroy@0 hipSetDevice@2 ", 0) == 0);
  m.unbind([&] {
    m.fused.release();
    m.tab.release();
  });
  F.cur = 0;
  CHECK(F.blocks.size() == live && F.streams == 0 && F.wrong_device_frees == 0);
}

// ---- the read side: where the streams lie -------------------------------------------------------------
struct StreamEntry {
  const void *stream;
  uint64_t len;
};

void test_stream_places() {
  const uintptr_t A = 0x7A00'0000'0000ull, H = 0x7B00'0000'0000ull;
  auto ptr = [](uintptr_t a) { return reinterpret_cast<const void *>(a); };
  fake_block(A, 4096, 0);
  fake_block(H, 4096, 0, true);
  StreamEntry e[3] = {{ptr(A), 4096}, {ptr(H), 0}, {ptr(A + 100), 100}};  // streams may overlap; no bytes, any address
  F.n.clear();
  CHECK(check_stream_places(e, 3, 0) == 0 && F.n["hipPointerGetAttributes"] == 1);
  e[2].len = 3997;
  char want[256];
  std::snprintf(want, sizeof(want), "entry 2: stream: 3997 bytes at %p run past the end of their device allocation", ptr(A + 100));
  CHECK(check_stream_places(e, 3, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  e[1].len = 8;
  std::snprintf(want, sizeof(want), "entry 1: stream: %p is not device memory", ptr(H));
  CHECK(check_stream_places(e, 3, 0) == HDFS_CRC32C_EINVAL && err_is(want));
  F.blocks.erase(A);
  F.blocks.erase(H);
}

}  // namespace

int main() {
  const int destroyed = F.plans_destroyed;
  test_last_error();
  test_engine_device();
  test_buffers();
  test_scratch();
  test_timing_events();
  test_table_pair();
  test_fused_state();
  test_placement();
  test_overlaps();
  test_batch_front_end();
  test_args_and_grid();
  test_tail_and_run();
  test_probed_run();
  test_outcomes();
  test_read_unlimited();
  test_walk_pieces();
  test_read_scratch();
  test_stream_places();
  CHECK(F.blocks.empty() && F.streams == 0 && F.events == 0 && F.wrong_device_frees == 0 && F.sticky == hipSuccess);
  CHECK(F.plans_destroyed - destroyed == 8);  // once for every call above that was given a plan
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
