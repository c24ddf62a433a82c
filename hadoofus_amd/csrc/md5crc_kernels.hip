// MD5CRC block checksums on gfx950: MD5 over each segment's chunk CRCs.
//
// One MD5 chain is serial, so the parallelism is one lane per segment.  A
// workgroup is one wave, so a batch's waves spread over CUs (1 024 blocks are
// 16 waves).  A lane consumes 64 B -- sixteen CRCs, one MD5 block -- per trip
// and loads the next trip's words before it runs the rounds.  Lanes of one
// wave have different trip counts; the loop runs under the exec mask until
// the longest is done.  No LDS, no atomics, no cross-lane traffic.
#include "md5_core.h"
#include "md5crc_internal.h"

namespace hdfs_md5crc {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// CRC arrays are global memory; saying so gives global_load, not flat_load.
typedef const __attribute__((address_space(1))) uint32_t *gwords;

// The sixteen words of MD5 block `blk` of a message of n CRC words at p,
// as stored (not yet in message order): whole blocks as four 16-byte loads --
// p is only 4-byte aligned, which the hardware's multi-dword global loads
// accept -- and the block the message ends in word by word, so nothing at or
// past p + n is read.  `pad` is the 0x80 word as it must be stored for the
// caller's byte order; words after it are zero.
__device__ __forceinline__ void load_words(gwords p, uint64_t n, uint32_t blk, uint32_t pad,
                                           uint32_t w[16]) {
  const uint64_t i0 = uint64_t(blk) * 16;
  if (i0 + 16 <= n) {
#pragma unroll
    for (int v = 0; v < 4; v++) {
      u32x4 x;
      __builtin_memcpy(&x, p + i0 + 4 * v, 16);
      w[4 * v + 0] = x.x;
      w[4 * v + 1] = x.y;
      w[4 * v + 2] = x.z;
      w[4 * v + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const uint64_t i = i0 + j;
      uint32_t x = i == n ? pad : 0u;
      if (i < n) x = p[i];
      w[j] = x;
    }
  }
}

}  // namespace

__global__ __launch_bounds__(64) void md5crc_block_kernel(const SegTab *__restrict__ tab, uint32_t nseg,
                                                          uint32_t *__restrict__ digests) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  if (s >= nseg) return;
  const SegTab t = tab[s];
  const gwords p = (gwords)t.crcs;
  const uint64_t n = t.nchunks;
  // Wire order is big-endian CRCs; the MD5 message word is little-endian.  A
  // stored wire-order u32, loaded, is the message word; a host-order one is
  // byte-swapped (one v_perm_b32 with a per-lane selector, identity for BE).
  const uint32_t sel = t.be ? 0x03020100u : 0x00010203u;
  const uint32_t pad = t.be ? 0x00000080u : 0x80000000u;
  const uint32_t nblk = uint32_t(md5_words_blocks(n));  // <= 2^28 + 1
  uint32_t st[4];
  md5_init(st);
  // cur: the block the rounds run on, in message order.  nxt: the following
  // block as loaded.  The loads are issued before the rounds and first
  // touched after them, so their latency hides under the rounds.  (cur is
  // made from nxt once before the loop, so that no load is pending on the
  // loop's entry edge: the compiler's wait-count bookkeeping would otherwise
  // wait for the in-loop loads at their issue.)
  uint32_t nxt[16], cur[16];
  load_words(p, n, 0, pad, nxt);
#pragma unroll
  for (int j = 0; j < 16; j++) cur[j] = __builtin_amdgcn_perm(0u, nxt[j], sel);
  for (uint32_t b = 0; b < nblk; b++) {
    if (b + 1 < nblk) load_words(p, n, b + 1, pad, nxt);
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = cur[j];
    if (b + 1 == nblk) {  // the message's length in bits, 64 bits: 32 * n
      m[14] = uint32_t(n << 5);
      m[15] = uint32_t(n >> 27);
    }
    md5_block(st, m);
#pragma unroll
    for (int j = 0; j < 16; j++) cur[j] = __builtin_amdgcn_perm(0u, nxt[j], sel);
  }
  u32x4 d;
  d.x = st[0];
  d.y = st[1];
  d.z = st[2];
  d.w = st[3];
  *reinterpret_cast<u32x4 *>(digests + 4 * size_t(s)) = d;
}

hipError_t launch_block_digests(const SegTab *tab, uint32_t nseg, uint32_t *digests, hipStream_t stream) {
  if (!nseg) return hipSuccess;
  hipLaunchKernelGGL(md5crc_block_kernel, dim3((nseg + 63) / 64), dim3(64), 0, stream, tab, nseg, digests);
  return hipGetLastError();
}

}  // namespace hdfs_md5crc
