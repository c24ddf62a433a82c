// Gather writes on gfx950: the CRCs of the chunks no in-place segment covers.
//
// One lane per gathered chunk, one wave per workgroup (a write of F fragments
// has about F such chunks, so its waves spread over CUs).  A lane walks its
// chunk's pieces in order and carries the CRC register from one piece to the
// next, as the reference's loop carries `crc` across iovecs
// (src/datanode.c:2840-2855).  Slicing-by-4 from a 4 KiB table in LDS, as
// crc32c_generic_kernel does for one buffer.  No atomics, no cross-lane
// traffic, no waiting on other workgroups.
//
// Bounds: a piece is read byte by byte up to the first 4-byte aligned address,
// then in aligned 16-byte and 4-byte loads while that many bytes are left, then
// byte by byte: no load starts before the piece or ends past it.  The only
// stores are the lanes' own CRC slots.
#include "writev_internal.h"

namespace hdfs_writev {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// Fragments are global memory; saying so gives global_load, not flat_load.
typedef const __attribute__((address_space(1))) uint8_t *gbytes;
typedef const __attribute__((address_space(1))) uint32_t *gwords;

__device__ __forceinline__ uint32_t crc_byte(const uint32_t *t, uint32_t r, uint32_t b) {
  return t[(r ^ b) & 0xffu] ^ (r >> 8);
}

// t[k * 256 + e]: byte e followed by k zero bytes (make_slicing4).
__device__ __forceinline__ uint32_t crc_word(const uint32_t *t, uint32_t r, uint32_t w) {
  w ^= r;
  return t[768 + (w & 0xffu)] ^ t[512 + ((w >> 8) & 0xffu)] ^ t[256 + ((w >> 16) & 0xffu)] ^ t[w >> 24];
}

}  // namespace

__global__ __launch_bounds__(64) void gather_chunks_kernel(const GChunk *__restrict__ ch, uint32_t ngathered,
                                                           const Piece *__restrict__ pc, uint32_t npieces,
                                                           const uint32_t *__restrict__ tab,
                                                           uint32_t *__restrict__ crcs, uint32_t nchunks) {
  __shared__ uint32_t t[kSliceWords];
  for (uint32_t i = threadIdx.x; i < kSliceWords; i += 64) t[i] = tab[i];
  __syncthreads();
  const uint32_t g = blockIdx.x * 64 + threadIdx.x;
  if (g >= ngathered) return;
  const GChunk c = ch[g];
  // the tables' sizes come from the host; a descriptor outside them is not followed
  if (c.slot >= nchunks || c.first > npieces || c.count > npieces - c.first) return;
  uint32_t r = 0xFFFFFFFFu;
  for (uint32_t k = 0; k < c.count; k++) {
    const Piece q = pc[c.first + k];
    gbytes p = (gbytes)q.p;
    uint32_t n = q.len;
    uint32_t head = uint32_t((4u - (reinterpret_cast<uintptr_t>(q.p) & 3u)) & 3u);  // bytes to alignment
    if (head > n) head = n;
    n -= head;
    for (; head; head--) r = crc_byte(t, r, *p++);
    for (; n >= 16; n -= 16, p += 16) {
      u32x4 x;
      __builtin_memcpy(&x, (gwords)p, 16);
      r = crc_word(t, r, x.x);
      r = crc_word(t, r, x.y);
      r = crc_word(t, r, x.z);
      r = crc_word(t, r, x.w);
    }
    for (; n >= 4; n -= 4, p += 4) r = crc_word(t, r, *(gwords)p);
    for (; n; n--) r = crc_byte(t, r, *p++);
  }
  crcs[c.slot] = __builtin_bswap32(~r);  // wire order
}

hipError_t launch_gather_chunks(const GChunk *ch, uint32_t ngathered, const Piece *pc, uint32_t npieces,
                                const uint32_t *tab, uint32_t *crcs, uint32_t nchunks, hipStream_t stream) {
  if (!ngathered) return hipSuccess;
  hipLaunchKernelGGL(gather_chunks_kernel, dim3((ngathered + 63) / 64), dim3(64), 0, stream, ch, ngathered, pc,
                     npieces, tab, crcs, nchunks);
  return hipGetLastError();
}

}  // namespace hdfs_writev
