// MD5CRC block digests from packet streams on gfx950 in three launches on one
// stream: probe_streams_kernel, check_headers_kernel, digest_streams_kernel
// (DESIGN.md section 23).  No byte of a packet's data is read.
//
// probe_streams_kernel is the read batch library's probe: one workgroup, thread
// e for entry e, read_batch_layout.h's probe_entry as it stands (no destination,
// so dst_cap is without limit, and no records).  Every regular entry's
// descriptor goes to its slot, and beside it the entry's CRC regions
// (md5crc_streams_internal.h: regions_of), the word count and the MD5 block
// count among them -- all of it from lengths.  There is no framing arithmetic
// here.
//
// check_headers_kernel is what the read batch's main launch does with a
// header, and nothing else of it: the probe framed only packet 0 and the tail,
// the digest will read CRC regions at PREDICTED positions, so every packet's
// header is first compared with the one the prediction composes
// (read_batch_header.h's verify_header: outpkt::put_out_header, plus the
// syncBlock bytes).  A wave takes a packet a step, packets g = w, w + W, ... of
// the regular entries, found with the lookup of wire_fused_batch_lookup.h on
// the packet-count prefix through the constant address space.  A mismatch makes
// the lane that saw it store 1 into its entry's status word: a plain vector
// store, every writer the same value.  No atomics, no spinning, no
// cross-workgroup dependence.  When every header matches, the chain of strides
// is the stream's own and the regions are where the main library's walk finds
// them.
//
// digest_streams_kernel is md5crc_block_kernel's organisation
// (md5crc_kernels.hip): one lane per entry, one wave per workgroup, md5_core.h's
// rounds and padding rules, the next trip's sixteen words loaded before the
// rounds and first touched after them, the state stored by one 16-byte store.
// A lane whose entry is flagged exits at once.  What is new is where the words
// come from: the cursor of md5crc_streams_lookup.h over the packets' CRC
// regions.  A block that lies in one region is four wide loads; one that
// begins in one packet and ends in another is taken word by word.
//
// ALIGNMENT.  A region lies at any byte address.  Lanes of one wave digest
// different entries, so a buffer range over exactly the region (range_of, a
// descriptor in scalar registers) would be one per lane: a waterfall loop over
// up to 64 descriptors for every load.  Global loads are per lane but want
// 4-byte alignment, so a misaligned word is two aligned words joined by a
// funnel shift (lookup.h: join); sixteen of them are seventeen aligned words.
// A block is kept as loaded and joined behind the rounds of the block ahead.
// The aligned words around a region overhang it by up to three bytes on either
// side: ahead lies the packet's header, behind its data, both inside the
// entry's consumed bytes -- except behind the last region of a stream that ends
// in a data packet of one or two bytes.  aligned_cover_ok tests exactly that
// against the descriptor's `consumed`, and the word is then read byte by byte.
//
// SAFETY.  Every trip count and address follows from the probe's descriptor,
// that is from lengths validated against len (nbody * stride + tail ==
// consumed <= len, every packet inside), never from stream bytes: no load
// leaves [stream, stream + consumed), and a corrupt stream costs a fallback,
// never an access out of range or an unbounded loop.  The header check's loads
// go through range_of over exactly the header's bytes.  Nothing is stored but
// the library's own tables.
#include "crc32c_frame.h"
#include "crc32c_outpkt.h"
#include "md5_core.h"
#include "md5crc_streams_internal.h"
#include "md5crc_streams_lookup.h"
#include "read_batch_header.h"
#include "read_batch_layout.h"
#include "read_batch_verify.h"
#include "wire_fused_batch_lookup.h"

namespace hdfs_md5crc_streams {

#define CAS __attribute__((address_space(4)))

using hdfs_md5crc::md5_block;
using hdfs_md5crc::md5_init;
using hdfs_read_batch::PacketAt;
using hdfs_read_batch::Round;
using hdfs_wire_fused::rfl;
using hdfs_wire_fused::u32x4;
using hdfs_wire_fused::write_of;

// ---- the probe ----------------------------------------------------------------------
struct DeviceBytes {
  const uint8_t *s;
  __host__ __device__ const uint8_t *operator()(uint64_t pos) const { return s + pos; }
};

__global__ __launch_bounds__(1024) void probe_streams_kernel(const Entry *__restrict__ in, uint32_t n, int proto,
                                                             uint32_t chunk_size, int ctype, Desc *__restrict__ desc,
                                                             Regions *__restrict__ reg, uint32_t *__restrict__ slot,
                                                             uint32_t *__restrict__ status,
                                                             uint32_t *__restrict__ pk0,
                                                             uint32_t *__restrict__ meta) {
  __shared__ uint32_t npk[kMaxEntries], at[kMaxEntries];
  const uint32_t e = threadIdx.x;
  Desc d;
  bool regular = false;
  if (e < n) {
    const Entry x = in[e];
    regular = hdfs_read_batch::probe_entry(DeviceBytes{x.stream}, x.len, ~uint64_t(0), proto, chunk_size, ctype, false,
                                           0, d);
    d.stream = x.stream;
    d.dst = nullptr;
    d.entry = e;
  }
  npk[e] = regular ? d.npk : 0u;
  __syncthreads();
  if (e == 0u) {
    const uint32_t nreg = hdfs_read_batch::prefix_regular(npk, n, at, pk0);
    meta[0] = nreg;
    meta[1] = pk0[nreg];
  }
  __syncthreads();
  if (e < n) {
    const uint32_t s = at[e];
    slot[e] = s;
    if (s != kNoSlot) {
      desc[s] = d;
      reg[s] = regions_of(d, d.stream, e);
      status[s] = 0u;
    }
  }
}

// ---- the header check ---------------------------------------------------------------
// Packet g of the regular entries as the comparison takes it (wave-uniform).
FUSED_DEV Round header_at(const CAS Desc *tab, const CAS uint32_t *pk0, uintptr_t status, uint32_t nw, uint32_t g,
                          uint32_t &k) {
  k = write_of(pk0, nw, g, k);
  const CAS Desc *p = tab + k;
  const uint32_t i = g - pk0[k], nbody = p->nbody;
  const bool body = i < nbody;
  const CAS PacketAt *t = p->tail + (body ? 0u : (i - nbody < kTailRegions ? i - nbody : 0u));
  const uint32_t dlen0 = p->dlen0;
  Round r;
  hdfs_wire_fused::Unit &u = r.u;
  u.p.wire_off = body ? uint64_t(i) * p->stride : t->stream_off;
  u.p.data_off = 0u;
  u.p.off = body ? p->off0 + int64_t(uint64_t(i) * dlen0) : t->off;
  u.p.seq = body ? p->seq0 + int64_t(i) : t->seq;
  u.p.dlen = body ? dlen0 : t->dlen;
  u.p.ncrc = hdfs_read_batch::crc_count(u.p.dlen);
  u.p.cidx = 0u;
  u.p.last = body ? p->last0 : t->last;
  r.sync = body ? p->sync0 : t->sync;
  u.hb = body ? p->hb0 : t->hb;
  u.h0 = reinterpret_cast<uintptr_t>(p->stream) + u.p.wire_off;
  u.c0 = u.d0 = u.src = u.dst = 0u;
  u.nfr = 0u;
  r.out0 = 0u;
  r.status = status + 4u * uintptr_t(k);
  return r;
}

__global__ __launch_bounds__(64 * kCheckWaves) void check_headers_kernel(const CAS Desc *dt, const CAS uint32_t *pk0,
                                                                        const CAS uint32_t *meta, uint32_t *status,
                                                                        uint32_t proto) {
  __shared__ uint32_t expect[kCheckWaves][16];  // the expected header, 33 bytes at most, one per wave
  const uint32_t nw = meta[0], total = meta[1];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  const uint32_t W = gridDim.x * kCheckWaves;  // <= 2^13; total < 2^29, so g + W does not wrap
  const uintptr_t st = reinterpret_cast<uintptr_t>(status);
  uint32_t k = 0u;
  for (uint32_t g = blockIdx.x * kCheckWaves + wave; g < total; g += W) {
    const Round r = header_at(dt, pk0, st, nw, g, k);
    hdfs_read_batch::flag(r, hdfs_read_batch::verify_header(expect[wave], proto, r, lane));
  }
}

// ---- the digest ---------------------------------------------------------------------
namespace {

// CRC regions are global memory; saying so gives global_load, not flat_load.
typedef const __attribute__((address_space(1))) uint32_t *gwords;
typedef const __attribute__((address_space(1))) uint8_t *gbytes;

// One word at base + off, any byte address, as loaded: the two aligned words
// around it (one word twice when it is aligned), or its bytes where the second
// word would leave the entry's bytes.
__device__ __forceinline__ void load_word(const Regions &r, uint64_t off, uint32_t &lo, uint32_t &hi, uint32_t &a) {
  const uint64_t A = r.base + off;
  a = uint32_t(A) & 3u;
  if (a != 0u && !aligned_cover_ok(r, off, a, 1u)) {
    const gbytes b = (gbytes)A;
    lo = by_bytes(b[0], b[1], b[2], b[3]);
    hi = a = 0u;
    return;
  }
  lo = *(gwords)lo_address(A);
  hi = *(gwords)hi_address(A);
}

// Sixteen words at base + off inside one region, as loaded: four 16-byte loads
// from the aligned address at or below (only 4-byte aligned, which the
// hardware's multi-dword global loads accept) and the seventeenth aligned word
// (the sixteenth again when the span is aligned).
__device__ __forceinline__ void load_span(const Regions &r, uint64_t off, Loaded &x) {
  const uint64_t A = r.base + off;
  const uint32_t a = uint32_t(A) & 3u;
  if (a != 0u && !aligned_cover_ok(r, off, a, kBlockWords)) {
    x.sh = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kBlockWords; j++) {
      uint32_t aj;
      load_word(r, off + 4u * j, x.lo[j], x.hi[j], aj);
      x.sh |= aj << (2u * j);
    }
    return;
  }
  const gwords p = (gwords)lo_address(A);
#pragma unroll
  for (int v = 0; v < 4; v++) {
    u32x4 q;
    __builtin_memcpy(&q, p + 4 * v, 16);
    x.lo[4 * v + 0] = q.x;
    x.lo[4 * v + 1] = q.y;
    x.lo[4 * v + 2] = q.z;
    x.lo[4 * v + 3] = q.w;
  }
  x.hi[kBlockWords - 1] = p[a ? kBlockWords : kBlockWords - 1u];
#pragma unroll
  for (uint32_t j = 0; j + 1u < kBlockWords; j++) x.hi[j] = x.lo[j + 1];
  x.sh = a * 0x55555555u;
}

// What block_words calls for a span and for a word.
struct SpanAt {
  const Regions &r;
  __device__ __forceinline__ void operator()(uint64_t off, Loaded &x) const { load_span(r, off, x); }
};
struct WordAt {
  const Regions &r;
  __device__ __forceinline__ void operator()(uint64_t off, uint32_t &lo, uint32_t &hi, uint32_t &a) const {
    load_word(r, off, lo, hi, a);
  }
};

}  // namespace

__global__ __launch_bounds__(64) void digest_streams_kernel(const Regions *__restrict__ reg,
                                                            const uint32_t *__restrict__ status,
                                                            const uint32_t *__restrict__ meta, uint32_t count,
                                                            uint32_t *__restrict__ digest) {
  const uint32_t s = blockIdx.x * 64 + threadIdx.x;
  const uint32_t n = meta ? meta[0] : count;
  if (s >= n || s >= count) return;
  if (status && status[s]) return;  // flagged by the header check: the host takes the fallback
  const Regions r = reg[s];
  Cursor c = start(r);
  const SpanAt span{r};
  const WordAt word{r};
  uint32_t st[4];
  md5_init(st);
  // cur: the block the rounds run on, joined.  nxt: the following block as
  // loaded.  The loads are issued before the rounds and first touched after
  // them -- the join of misaligned words included -- so their latency hides
  // under the rounds (md5crc_kernels.hip).  A CRC's wire bytes are the message's
  // bytes, so a joined word is the message word as it is.
  Loaded nxt;
  uint32_t cur[kBlockWords];
  block_words(r, c, 0u, span, word, nxt);
  message_words(nxt, cur);
  for (uint32_t b = 0; b < r.nblk; b++) {
    if (b + 1 < r.nblk) block_words(r, c, b + 1u, span, word, nxt);
    uint32_t m[16];
#pragma unroll
    for (int j = 0; j < 16; j++) m[j] = cur[j];
    if (b + 1 == r.nblk) {  // the message's length in bits, 64 bits: 32 * nwords
      m[14] = uint32_t(r.nwords << 5);
      m[15] = uint32_t(r.nwords >> 27);
    }
    md5_block(st, m);
    message_words(nxt, cur);
  }
  u32x4 d;
  d.x = st[0];
  d.y = st[1];
  d.z = st[2];
  d.w = st[3];
  *reinterpret_cast<u32x4 *>(digest + 4 * size_t(s)) = d;
}

// ---- the fallback's gather ------------------------------------------------------------
// Record k's bytes, a packet's CRC region as hdfs_crc32c_parse_packets framed
// it, to the library's scratch: byte loads and byte stores, any address.
__global__ __launch_bounds__(kGatherThreads) void gather_regions_kernel(const GatherRec *__restrict__ recs,
                                                                        uint8_t *__restrict__ scratch) {
  const GatherRec k = recs[blockIdx.x];
  const uint8_t *src = reinterpret_cast<const uint8_t *>(uintptr_t(k.src));
  for (uint32_t i = threadIdx.x; i < k.bytes; i += kGatherThreads) scratch[k.dst + i] = src[i];
}

// ---- launches -------------------------------------------------------------------------
hipError_t launch_probe_streams(void *tables, uint32_t n, int proto, uint32_t chunk_size, int ctype,
                                hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(probe_streams_kernel, dim3(1), dim3(kMaxEntries), 0, stream,
                     reinterpret_cast<const Entry *>(b + t.in), n, proto, chunk_size, ctype,
                     reinterpret_cast<Desc *>(b + t.desc), reinterpret_cast<Regions *>(b + t.reg),
                     reinterpret_cast<uint32_t *>(b + t.slot), reinterpret_cast<uint32_t *>(b + t.status),
                     reinterpret_cast<uint32_t *>(b + t.pk0), reinterpret_cast<uint32_t *>(b + t.meta));
  return hipGetLastError();
}

hipError_t launch_check_headers(void *tables, uint32_t n, uint32_t proto, uint32_t groups, hipStream_t stream) {
  if (!tables || !n || n > kMaxEntries || !groups || groups > kCheckMaxGroups) return hipErrorInvalidValue;
  const Tables t(n);
  uint8_t *b = static_cast<uint8_t *>(tables);
  hipLaunchKernelGGL(check_headers_kernel, dim3(groups), dim3(64 * kCheckWaves), 0, stream,
                     (const CAS Desc *)(b + t.desc), (const CAS uint32_t *)(b + t.pk0),
                     (const CAS uint32_t *)(b + t.meta), reinterpret_cast<uint32_t *>(b + t.status), proto);
  return hipGetLastError();
}

hipError_t launch_digest_streams(const Regions *reg, const uint32_t *status, const uint32_t *meta, uint32_t count,
                                 uint32_t *digest, hipStream_t stream) {
  if (!reg || !digest || !count) return hipErrorInvalidValue;
  hipLaunchKernelGGL(digest_streams_kernel, dim3((count + 63) / 64), dim3(64), 0, stream, reg, status, meta, count,
                     digest);
  return hipGetLastError();
}

hipError_t launch_gather_regions(const GatherRec *recs, uint32_t nrec, uint8_t *scratch, hipStream_t stream) {
  if (!nrec) return hipSuccess;
  if (!recs || !scratch) return hipErrorInvalidValue;
  hipLaunchKernelGGL(gather_regions_kernel, dim3(nrec), dim3(kGatherThreads), 0, stream, recs, scratch);
  return hipGetLastError();
}

}  // namespace hdfs_md5crc_streams
