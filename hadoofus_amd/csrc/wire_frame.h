// One packet of a write framed into its wire stream on gfx950: the body that
// frame_packets_kernel (wire_kernels.hip, one write per launch) and
// frame_batch_kernel (wire_batch_kernels.hip, a batch of writes per launch)
// both run, so there is one definition of it.  frame_gather_kernel
// (wirev_kernels.hip, the data in a list of fragments) runs its region copy
// and its CRC-and-header part.  Device code; hipcc only.
//
// A packet is three regions of the stream, each starting and ending at any
// byte address (a full packet's stride is odd): the header, which the
// workgroup composes itself (outpkt::put_out_header into LDS, from the closed
// form packet_at); the chunk CRCs, copied from the CRC array the compute plan
// filled, already in wire byte order; the data, copied from the write's
// buffer.  A region [d, e) is cut at the destination's 16-B grid: the blocks
// wholly inside it (its interior) go out as one 16-B aligned dwordx4 store
// each, the fewer than 16 bytes ahead of the first and behind the last as one
// byte store per lane.  An interior block's 16 source bytes sit at the same
// phase for the whole region (destination blocks are 16 B apart, so are their
// sources): the lane loads the dword-aligned window around them -- four
// dwords, and a fifth only when the phase is not 0, so every dword loaded
// holds a byte of the region's source -- and funnel-shifts it into place
// (v_alignbyte_b32).
//
// Every byte of the packet is stored exactly once: the regions tile it, a
// region's head, interior blocks and tail tile the region, slice 0 alone
// stores the header, the CRCs and every region's head and tail, and the
// data's interior blocks are dealt to the slices in contiguous runs.  No
// destination byte is read, nothing outside the packet is stored.  No
// atomics, no waiting on other workgroups; LDS holds the 31 header bytes.
//
// The interior is software-pipelined as copy_staged of the main library is:
// the loads of a lane's next kUnits blocks are issued ahead of the stores of
// its current ones.
#ifndef HADOOFUS_WIRE_FRAME_H
#define HADOOFUS_WIRE_FRAME_H

#include "crc32c_outpkt.h"
#include "wire_internal.h"

namespace hdfs_wire {
namespace frame {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// The write, the CRC array and the stream are global memory; saying so gives
// global_load / global_store, not flat_*.
typedef const __attribute__((address_space(1))) uint8_t *gbytes;
typedef const __attribute__((address_space(1))) uint32_t *gwords;
typedef __attribute__((address_space(1))) uint8_t *gout;
typedef __attribute__((address_space(1))) u32x4 *gout16;

#define WIRE_DEV static __device__ __forceinline__

constexpr int kUnits = 4;  // 16-B blocks a lane has in flight per batch

template <bool SC1>
WIRE_DEV void store16(uintptr_t D, u32x4 v) {
  if (SC1)  // s_nop 1: a store of more than 64 bits reads its data registers late; the compiler pads its own
            // stores against the next write of them, not one inside a string
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(D), "v"(v) : "memory");
  else
    *(gout16)D = v;
}

WIRE_DEV void store8(uintptr_t x, uint32_t v) { *(gout)x = uint8_t(v); }

// Bytes [sh, sh + 16) of the five-dword window w[0..4] (sh < 4).
WIRE_DEV u32x4 shift_window(u32x4 w, uint32_t w4, uint32_t sh) {
  u32x4 v;
  v.x = __builtin_amdgcn_alignbyte(w.y, w.x, sh);
  v.y = __builtin_amdgcn_alignbyte(w.z, w.y, sh);
  v.z = __builtin_amdgcn_alignbyte(w.w, w.z, sh);
  v.w = __builtin_amdgcn_alignbyte(w4, w.w, sh);
  return v;
}

// A region's cut at the destination's 16-B grid: head [d, he), interior
// [he, ts) (whole blocks), tail [ts, e).  A region inside one block is all
// head.
struct Cut {
  uintptr_t he, ts;
};
WIRE_DEV Cut cut16(uintptr_t d, uintptr_t e) {
  const uintptr_t up = (d + 15u) & ~uintptr_t(15), dn = e & ~uintptr_t(15);
  Cut c;
  c.he = up < e ? up : e;
  c.ts = dn > c.he ? dn : c.he;
  return c;
}

struct Ld {
  u32x4 w;
  uint32_t w4;
};

// The window of interior block u: a is the dword-aligned address at or below
// the source of interior byte 0, sh (uniform) the bytes between them.
WIRE_DEV void issue(Ld &x, gbytes a, uint32_t sh, uint32_t u, uint32_t u1) {
  if (u >= u1) return;
  gwords p = (gwords)(a + 16u * size_t(u));
  __builtin_memcpy(&x.w, p, 16);  // 4-byte aligned: one global_load_dwordx4
  x.w4 = sh ? p[4] : 0u;          // only when it holds one of the block's bytes
}

// Region [d, e) of the stream <- src[0, e - d), global memory.  edges: this
// workgroup stores the head and the tail; the interior blocks are dealt to
// `slices` workgroups in contiguous runs, this one taking run `slice`.
template <bool SC1>
WIRE_DEV void copy_region(gbytes src, uintptr_t d, uintptr_t e, bool edges, uint32_t slice, uint32_t slices,
                          uint32_t tid) {
  const Cut c = cut16(d, e);
  if (edges) {  // lanes 0-14 the head's bytes, lanes 16-30 the tail's
    if (tid < c.he - d) store8(d + tid, src[tid]);
    if (tid >= 16u && tid - 16u < e - c.ts) store8(c.ts + (tid - 16u), src[(c.ts - d) + (tid - 16u)]);
  }
  const uint32_t n = uint32_t((c.ts - c.he) >> 4);  // a region is at most a packet's data: 4 096 blocks
  const uint32_t per = (n + slices - 1u) / slices;
  const uint32_t u0 = slice * per < n ? slice * per : n, u1 = u0 + per < n ? u0 + per : n;
  const uintptr_t sa = reinterpret_cast<uintptr_t>(src) + (c.he - d);
  const uint32_t sh = uint32_t(sa & 3u);
  gbytes a = (gbytes)(sa - sh);
  Ld cur[kUnits], nxt[kUnits];
#pragma unroll
  for (int k = 0; k < kUnits; k++) issue(cur[k], a, sh, u0 + tid + 256u * uint32_t(k), u1);
  for (uint32_t ub = u0 + tid; ub < u1; ub += 256u * kUnits) {
#pragma unroll
    for (int k = 0; k < kUnits; k++) issue(nxt[k], a, sh, ub + 256u * uint32_t(kUnits + k), u1);
#pragma unroll
    for (int k = 0; k < kUnits; k++) {
      const uint32_t u = ub + 256u * uint32_t(k);
      if (u < u1) store16<SC1>(c.he + 16u * uintptr_t(u), shift_window(cur[k].w, cur[k].w4, sh));
    }
#pragma unroll
    for (int k = 0; k < kUnits; k++) cur[k] = nxt[k];
  }
}

// Region [d, d + hb) of the stream <- the header bytes in LDS (hb <= 31, so
// 8 words: a block's window never reaches past word 7).
template <bool SC1>
WIRE_DEV void copy_header(const uint32_t *lh, uintptr_t d, uint32_t hb, uint32_t tid) {
  const uintptr_t e = d + hb;
  const Cut c = cut16(d, e);
  const uint8_t *lb = reinterpret_cast<const uint8_t *>(lh);
  if (tid < c.he - d) store8(d + tid, lb[tid]);
  if (tid >= 16u && tid - 16u < e - c.ts) store8(c.ts + (tid - 16u), lb[(c.ts - d) + (tid - 16u)]);
  if (tid >= 32u && tid - 32u < uint32_t((c.ts - c.he) >> 4)) {
    const uint32_t o = uint32_t(c.he - d) + 16u * (tid - 32u), sh = o & 3u;
    const uint32_t *p = lh + (o >> 2);
    const u32x4 w = {p[0], p[1], p[2], p[3]};
    store16<SC1>(c.he + 16u * uintptr_t(tid - 32u), shift_window(w, sh ? p[4] : 0u, sh));
  }
}

// What slice 0 alone does for packet p of write w, whose first byte lies at
// h0: the CRC region from the plan's array, then the header, composed into
// the workgroup's 8 words of LDS at lh.  A whole workgroup of 256 threads.
template <bool SC1>
WIRE_DEV void frame_crcs_and_header(const Write &w, const Pkt &p, uintptr_t h0, uint32_t *lh, uint32_t tid) {
  const uintptr_t c0 = h0 + w.hb, d0 = c0 + 4u * uintptr_t(p.ncrc);
  if (p.ncrc) copy_region<SC1>((gbytes)(w.crc + p.cidx), c0, d0, true, 0u, 1u, tid);
  if (tid == 0)
    hdfs_crc32c::outpkt::put_out_header(reinterpret_cast<uint8_t *>(lh), int(w.proto), p.off, p.seq, p.last != 0u,
                                        int32_t(p.dlen), p.ncrc);
  __syncthreads();
  copy_header<SC1>(lh, h0, w.hb, tid);
}

// Slice `slice` of `slices` of packet i (i < w.npk) of write w, by a whole
// workgroup of 256 threads; lh: 8 words of LDS of the workgroup.  Every
// argument but tid is uniform across the workgroup.
template <bool SC1>
WIRE_DEV void frame_packet(const Write &w, uint32_t i, uint32_t slice, uint32_t slices, uint32_t *lh, uint32_t tid) {
  const Pkt p = packet_at(w, i);
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(w.wire) + p.wire_off;
  const uintptr_t d0 = h0 + w.hb + 4u * uintptr_t(p.ncrc), d1 = d0 + p.dlen;
  copy_region<SC1>((gbytes)(w.data + p.data_off), d0, d1, slice == 0u, slice, slices, tid);
  if (slice != 0u) return;
  frame_crcs_and_header<SC1>(w, p, h0, lh, tid);
}

}  // namespace frame
}  // namespace hdfs_wire

#endif  // HADOOFUS_WIRE_FRAME_H
