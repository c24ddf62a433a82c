// libhadoofus_md5crc.so: entry points of include/hadoofus_md5crc.h.
//
// A companion of libhadoofus_crc32c.so, not a second engine: the device is
// the one that library is bound to (hdfs_crc32c_init /
// hdfs_crc32c_bound_device, its public API), and both share one HIP runtime.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>
#include <vector>

#include "companion_support.h"
#include "hadoofus_md5crc.h"
#include "md5_core.h"
#include "md5crc_internal.h"

namespace hdfs_md5crc {
namespace {

using namespace hdfs_companion;

// The segment table and the digests of one call, on the engine's device;
// grown on demand, kept between calls (an allocation per call would cost
// more than the launch).  The calls run on the caller's stream, so this
// scratch has none of its own.  Calls hold g_mu from the upload to the final
// synchronise, so one call's table is never overwritten under its kernel.
std::mutex g_mu;
DeviceBuffer g_scratch;
int g_scratch_dev = -1;

int scratch(int dev, size_t bytes, void **out) {
  if (g_scratch_dev != dev) g_scratch.release();
  g_scratch_dev = dev;
  const int rc = g_scratch.reserve(bytes, kScratchFloor);
  *out = g_scratch.p;
  return rc;
}

bool device_accessible(const void *p) { return placement(p).device_ptr != nullptr; }

int seg_ctype(uint32_t flags) {
  return (flags & HDFS_CRC32C_SEG_CRC32) ? HDFS_CRC32C_CSUM_CRC32 : HDFS_CRC32C_CSUM_CRC32C;
}

// Validate segment i and describe it for the kernel.
int fill_seg(const hdfs_crc32c_segment &in, size_t i, SegTab &t) {
  if (in.flags & ~(HDFS_CRC32C_SEG_BE | HDFS_CRC32C_SEG_RAW | HDFS_CRC32C_SEG_CRC32))
    return fail(HDFS_CRC32C_EINVAL, "segment %zu: unknown flags 0x%x", i, in.flags);
  if (in.flags & HDFS_CRC32C_SEG_RAW)
    return fail(HDFS_CRC32C_EINVAL, "segment %zu: MD5CRC is over finished CRCs, not raw registers (SEG_RAW)", i);
  if (in.crc_init) return fail(HDFS_CRC32C_EINVAL, "segment %zu: MD5CRC needs chunk CRCs started from 0", i);
  if (!in.chunk_size) return fail(HDFS_CRC32C_EINVAL, "segment %zu: chunk_size 0", i);
  const uint64_t nch = in.len / in.chunk_size + (in.len % in.chunk_size ? 1 : 0);
  if (nch > 0xFFFFFFFFull) return fail(HDFS_CRC32C_EINVAL, "segment %zu: more than 2^32 - 1 chunks", i);
  if (nch) {
    if (!in.crcs || (reinterpret_cast<uintptr_t>(in.crcs) & 3))
      return fail(HDFS_CRC32C_EINVAL, "segment %zu: crcs is NULL or not 4-byte aligned", i);
    if (!device_accessible(in.crcs))
      return fail(HDFS_CRC32C_EINVAL, "segment %zu: crcs is not device-accessible memory", i);
  }
  t.crcs = nch ? static_cast<const uint32_t *>(in.crcs) : nullptr;
  t.nchunks = uint32_t(nch);
  t.be = (in.flags & HDFS_CRC32C_SEG_BE) ? 1u : 0u;
  return HDFS_CRC32C_OK;
}

uint32_t le32(const uint8_t *p) {
  return uint32_t(p[0]) | uint32_t(p[1]) << 8 | uint32_t(p[2]) << 16 | uint32_t(p[3]) << 24;
}

void md5_bytes(const void *buf, uint64_t len, uint8_t out[16]) {
  const uint8_t *p = static_cast<const uint8_t *>(buf);
  uint32_t st[4], m[16];
  md5_init(st);
  uint64_t left = len;
  for (; left >= 64; left -= 64, p += 64) {
    for (int j = 0; j < 16; j++) m[j] = le32(p + 4 * j);
    md5_block(st, m);
  }
  uint8_t tail[128] = {0};
  if (left) std::memcpy(tail, p, size_t(left));
  tail[left] = 0x80;
  const size_t tl = left < 56 ? 64 : 128;
  const uint64_t bits = len << 3;
  for (int k = 0; k < 8; k++) tail[tl - 8 + k] = uint8_t(bits >> (8 * k));
  for (size_t o = 0; o < tl; o += 64) {
    for (int j = 0; j < 16; j++) m[j] = le32(tail + o + 4 * j);
    md5_block(st, m);
  }
  for (int j = 0; j < 4; j++)
    for (int k = 0; k < 4; k++) out[4 * j + k] = uint8_t(st[j] >> (8 * k));
}

bool ctype_ok(int ctype) { return ctype == HDFS_CRC32C_CSUM_CRC32 || ctype == HDFS_CRC32C_CSUM_CRC32C; }

}  // namespace
}  // namespace hdfs_md5crc

using namespace hdfs_md5crc;

extern "C" {

int hdfs_md5crc_abi_version(void) { return HDFS_MD5CRC_ABI_VERSION; }

const char *hdfs_md5crc_last_error(void) { return last_error(); }

int hdfs_md5crc_md5_host(const void *buf, uint64_t len, void *out16) {
  if (!out16 || (len && !buf)) return fail(HDFS_CRC32C_EINVAL, "null buffer / out");
  md5_bytes(buf, len, static_cast<uint8_t *>(out16));
  return HDFS_CRC32C_OK;
}

int hdfs_md5crc_block_digests(const hdfs_crc32c_segment *segs, size_t nseg, void *stream, void *md5_out) {
  if (!nseg) return HDFS_CRC32C_OK;
  if (!segs || !md5_out) return fail(HDFS_CRC32C_EINVAL, "null segments / md5_out");
  if (nseg > (size_t(1) << 26)) return fail(HDFS_CRC32C_EINVAL, "too many segments");
  int dev = -1;
  int rc = engine_device(&dev);
  if (rc) return rc;
  DeviceGuard g(dev);
  std::vector<SegTab> tab(nseg);
  for (size_t i = 0; i < nseg; i++) {
    rc = fill_seg(segs[i], i, tab[i]);
    if (rc) return rc;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mu);
  void *d = nullptr;
  rc = scratch(dev, nseg * (sizeof(SegTab) + HDFS_MD5CRC_LEN), &d);
  if (rc) return rc;
  SegTab *d_tab = static_cast<SegTab *>(d);
  uint32_t *d_out = reinterpret_cast<uint32_t *>(d_tab + nseg);  // 16-byte aligned: sizeof(SegTab) == 16
  hipError_t e = hipMemcpyAsync(d_tab, tab.data(), nseg * sizeof(SegTab), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = launch_block_digests(d_tab, uint32_t(nseg), d_out, st);
  if (e == hipSuccess) e = hipMemcpyAsync(md5_out, d_out, nseg * HDFS_MD5CRC_LEN, hipMemcpyDefault, st);
  // always: the table and the digests must be out of use before the lock goes
  return sync_and_report(st, e, HDFS_CRC32C_OK, nullptr, "block digests");
}

int hdfs_md5crc_file_from_blocks(const void *block_md5s, size_t nblocks, uint32_t bytes_per_crc,
                                 uint64_t crc_per_block, int ctype, hdfs_md5crc_file_checksum *out) {
  if (!out || (nblocks && !block_md5s)) return fail(HDFS_CRC32C_EINVAL, "null block digests / out");
  if (!ctype_ok(ctype)) return fail(HDFS_CRC32C_EINVAL, "checksum type %d is neither CRC32 nor CRC32C", ctype);
  if (bytes_per_crc > 0x7FFFFFFFu) return fail(HDFS_CRC32C_EINVAL, "bytes_per_crc does not fit the s32 wire field");
  if (nblocks > SIZE_MAX / HDFS_MD5CRC_LEN) return fail(HDFS_CRC32C_EINVAL, "too many blocks");
  std::memset(out, 0, sizeof(*out));
  out->bytes_per_crc = bytes_per_crc;
  out->ctype = uint32_t(ctype);
  out->crc_per_block = crc_per_block;
  md5_bytes(block_md5s, uint64_t(nblocks) * HDFS_MD5CRC_LEN, out->md5);
  return HDFS_CRC32C_OK;
}

int hdfs_md5crc_file_checksum_dev(const hdfs_crc32c_segment *blocks, size_t nblocks, void *stream,
                                  hdfs_md5crc_file_checksum *out) {
  if (!blocks || !nblocks || !out) return fail(HDFS_CRC32C_EINVAL, "null or empty block list / out");
  const uint32_t cs = blocks[0].chunk_size;
  const int ctype = seg_ctype(blocks[0].flags);
  for (size_t i = 1; i < nblocks; i++) {
    if (blocks[i].chunk_size != cs)
      return fail(HDFS_CRC32C_EINVAL, "block %zu: chunk_size %u differs from block 0's %u", i, blocks[i].chunk_size, cs);
    if (seg_ctype(blocks[i].flags) != ctype)
      return fail(HDFS_CRC32C_EINVAL, "block %zu: CRC32 / CRC32C mixed in one file", i);
  }
  std::vector<uint8_t> md5s(nblocks * HDFS_MD5CRC_LEN);
  int rc = hdfs_md5crc_block_digests(blocks, nblocks, stream, md5s.data());
  if (rc) return rc;
  const uint64_t cpb = nblocks > 1 ? blocks[0].len / cs + (blocks[0].len % cs ? 1 : 0) : 0;
  return hdfs_md5crc_file_from_blocks(md5s.data(), nblocks, cs, cpb, ctype, out);
}

int hdfs_md5crc_algorithm_name(const hdfs_md5crc_file_checksum *c, char *buf, size_t len) {
  if (!c || !buf || !len) return fail(HDFS_CRC32C_EINVAL, "null checksum / buffer");
  if (!ctype_ok(int(c->ctype))) return fail(HDFS_CRC32C_EINVAL, "checksum type %u is neither CRC32 nor CRC32C", c->ctype);
  const int n = std::snprintf(buf, len, "MD5-of-%lluMD5-of-%u%s", static_cast<unsigned long long>(c->crc_per_block),
                              c->bytes_per_crc, c->ctype == HDFS_CRC32C_CSUM_CRC32 ? "CRC32" : "CRC32C");
  if (n < 0 || size_t(n) >= len) return fail(HDFS_CRC32C_EINVAL, "name needs %d bytes, buffer has %zu", n + 1, len);
  return HDFS_CRC32C_OK;
}

int hdfs_md5crc_file_bytes(const hdfs_md5crc_file_checksum *c, void *out28) {
  if (!c || !out28) return fail(HDFS_CRC32C_EINVAL, "null checksum / out");
  uint8_t *o = static_cast<uint8_t *>(out28);
  for (int k = 0; k < 4; k++) o[k] = uint8_t(c->bytes_per_crc >> (8 * (3 - k)));
  for (int k = 0; k < 8; k++) o[4 + k] = uint8_t(c->crc_per_block >> (8 * (7 - k)));
  std::memcpy(o + 12, c->md5, HDFS_MD5CRC_LEN);
  return HDFS_CRC32C_OK;
}

}  // extern "C"
