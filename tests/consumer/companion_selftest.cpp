// CPU self-test of the companion libraries' shared host support
// (hadoofus_amd/csrc/companion_support.h, and grid_segments / timed_frame_run
// of wire_layout.h) against a fake HIP runtime and a fake engine, both
// defined here: the program is not linked to the HIP runtime.  The fakes count
// and log every call, remember the current device and can be told to fail, so
// the checks cover what the GPU tests cannot: failed allocations and streams,
// a device change, the exact runtime calls of a warm call.  Prints
// "N failures".
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
  bool any_range = false;  // an address inside no block is reported as part of the lowest block
  int wrong_device_frees = 0, streams = 0;
  // the fake engine
  int init_rc = 0, bound_rc = 0, exec_rc = 0, engine_dev = 0, plans_destroyed = 0;
  std::string engine_text = "engine text";

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

}  // namespace

int main() {
  const int destroyed = F.plans_destroyed;
  test_last_error();
  test_engine_device();
  test_buffers();
  test_scratch();
  test_placement();
  test_args_and_grid();
  test_tail_and_run();
  CHECK(F.blocks.empty() && F.streams == 0 && F.wrong_device_frees == 0 && F.sticky == hipSuccess);
  CHECK(F.plans_destroyed - destroyed == 8);  // once for every call above that was given a plan
  std::printf("%d failures\n", g_fail);
  return g_fail ? 1 : 0;
}
