// The wire streams of a batch of writes, each held in a list of device
// fragments, on gfx950 in ONE pass over the data and ONE launch:
// frame_fused_gather_batch_kernel.
//
// The grid, the walk and the round are frame_fused_batch_kernel's
// (wire_fused_batch_kernels.hip), the round the one definition of
// wire_fused_round.h: min(CUs, packets) workgroups of 16 waves, workgroup b
// takes global packets g = b, b + G, ... of the whole batch, wave v takes round
// v (4 KiB, eight chunks) of the workgroup's packet, wave 0 composes and stores
// the header and does the chunk shorter than 512 B.  The table image is filled
// once per workgroup, behind the only barrier; two register sets take turns;
// the next packet's loads are issued ahead of the current round's stores.
//
// The data source is frame_fused_gather_kernel's (wirev_fused_kernels.hip):
// every write's entry has data == NULL, so unit_of's u.src is the round's
// first byte ra in the write's fragments' concatenation.  A round with a full
// chunk finds its fragment in the write's slice of the fragment table
// (frag_of); if its full chunks end inside that fragment it is the fast round,
// otherwise load_round runs through an empty range and seam_round assembles
// the same registers piece by piece.  The chunk shorter than 512 B is
// ragged_gather's.  load_unit_at below is that file's load_unit with the
// write and the slice looked up first: the few similar lines are the price of
// leaving that kernel's file as it is.
//
// What connects the two lookups is wirev_fused_batch_lookup.h's, shared with
// the host self-test: the write of a global packet (seek_write), which resets
// the wave's fragment hint when the write changes; the write's slice
// (slice_of) and the fragment (seek_frag), asked only by a round with a full
// chunk; and the cursor copy `kc` that gives the ragged chunk the current
// packet's write and hint after the next packet's lookups have moved on.
// Everything but the loads' lane offsets is wave-uniform, and all four tables
// are read through the constant address space: scalar loads, scalar loops.
//
// Invariants.  Every byte of every [wire, wire + wire_len) is stored exactly
// once, as frame_fused_batch_kernel stores it; no destination byte is read; no
// store falls outside a write's own stream.  Every vector load goes through a
// range over exactly the bytes of one fragment it may touch, so only the
// fragments' own bytes are read.  The fragment table is read inside the
// current write's slice only, pk0 and fr0 at [0, nw], the write table at
// [0, nw - 1].  No atomics, no cross-workgroup dependence, no spinning.
//
// The registers, LDS and waits the compiler chose are written up in DESIGN.md
// section 19.
#include "wire_fused_round.h"
#include "wirev_fused_batch_internal.h"
#include "wirev_fused_batch_lookup.h"

namespace hdfs_wirev_fused_batch {

using namespace hdfs_wirev_fused;  // the fragment table, the seamed round and the ragged chunk: wirev_fused_internal.h's

// The batch's four tables, as the kernel reads them.
struct Tabs {
  FragTab ft;
  const CAS Write *wt;
  const CAS uint32_t *pk0, *fr0;
  uint32_t nw, total;
};

// The wave's round of global packet g with its write, its slice and its source
// found, and its loads issued into v.  c: the write and the fragment the wave
// found last, updated.  Everything but the loads' lane offsets is wave-uniform.
FUSED_DEV Unit load_unit_at(u32x4 (&v)[4], const Tabs &t, uint32_t g, uint32_t wave, Cursor &c, uint32_t lo) {
  const bool in = seek_write(t.pk0, t.nw, t.total, g, c);
  const CAS Write *p = t.wt + c.kw;
  const Write w{p->data, p->crc, p->wire, p->len, p->off, p->seq, p->n0, p->npk, p->hb, p->proto, p->csum, p->finish,
                p->slices};
  Unit u = unit_of(w, in ? g - t.pk0[c.kw] : w.npk, wave);  // i == npk: no packet; w.data == NULL: u.src is the round's first byte in the write
  const uint64_t ra = u.src;
  bool seamed = false;
  FragTab ft = t.ft;
  uint32_t nf = 0u, k = 0u;
  if (u.nfr) {  // ra < len: the only rounds that look a slice or a fragment up
    const Slice s = slice_of(t.fr0, c.kw);
    ft += s.first;
    nf = s.nf;
    k = seek_frag(AtOf{ft}, nf, ra, c);
    const uint64_t fa = ft[k].at, fe = ft[k + 1u].at;  // k + 1 <= nf: the write's sentinel
    seamed = ra + u.nfr * kChunk > fe;
    u.src = reinterpret_cast<uintptr_t>(ft[k].base) + uintptr_t(ra - fa);
  }
  Unit ul = u;
  if (seamed) ul.nfr = 0u;  // an empty range: zeros, nothing read
  load_round(v, ul, lo);
  if (seamed) seam_round(v, ft, nf, k, ra, u.nfr * kChunk, lo);
  return u;
}

template <bool CSUM>
__global__ __launch_bounds__(1024) void frame_fused_gather_batch_kernel(FragTab ft, const CAS Write *wt,
                                                                        const CAS uint32_t *pk0, uint32_t nw,
                                                                        uint32_t total, uint32_t proto,
                                                                        const uint32_t *__restrict__ tab) {
  extern __shared__ uint32_t lds[];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = rfl(tid >> 6);
  uint32_t *hdr = lds;
  uint32_t init512 = 0u;
  if (CSUM) {
    hdr = lds + crc::kImageWords;
    fill_image(lds, tab, tid);
    init512 = tab[crc::kCompactInit + kChunk];
    __syncthreads();
  }
  const uint32_t lo = 64u * (lane & 15u) + 16u * (lane >> 4);
  const uint32_t G = gridDim.x;
  const Tabs t{ft, wt, pk0, pk0 + nw + 1u, nw, total};
  uint32_t g = blockIdx.x;
  Cursor c;
  // Two register sets take turns, as in frame_fused_batch_kernel.
  u32x4 ra[4], rb[4];
  Unit u = load_unit_at(ra, t, g, wave, c, lo);
  Cursor kc = c;  // as the current packet's lookups left it: its write, and a fragment no later than that of its chunk shorter than 512 B
  auto step = [&](const u32x4(&cur)[4], u32x4(&nxt)[4]) {
    const Unit un = load_unit_at(nxt, t, g + G, wave, c, lo);  // the next packet's loads, ahead of this round's stores; g + G < 2^32: total < 2^29, G <= 1024
    store_round(cur, u, lo);
    crc_round<CSUM>(lds, cur, u, wave, lane, init512);
    if (wave == 0u) {
      header(hdr, proto, u, lane);
      const Slice s = slice_of(t.fr0, kc.kw);  // the current packet's slice, not the one the loads above moved to
      ragged_gather<CSUM>(lds, tab, t.ft + s.first, s.nf, kc.kf, u, lane);
    }
    kc = c;
    g += G;
    u = un;
  };
  while (g < total) {
    step(ra, rb);
    if (g >= total) break;
    step(rb, ra);
  }
}

hipError_t prepare_frame_fused_gather_batch() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&frame_fused_gather_batch_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kHdrWords) * sizeof(uint32_t)));
}

hipError_t launch_frame_fused_gather_batch(const void *tables, uint32_t nw, uint32_t nfe, uint32_t total_pk,
                                           uint32_t proto, bool csum, const uint32_t *crc_tab, uint32_t groups,
                                           hipStream_t stream) {
  if (!total_pk) return hipSuccess;
  if (!tables || !nw || nw > total_pk || nfe < nw || total_pk > 0x7FFFFFFFu / 4u || !groups ||
      groups > kBatchMaxGroups || (csum && !crc_tab))
    return hipErrorInvalidValue;
  const Tables at = tables_of(nw, nfe);
  const uint8_t *b = static_cast<const uint8_t *>(tables);
  const FragTab ft = (FragTab) reinterpret_cast<const Frag *>(b);
  const CAS Write *wt = (const CAS Write *)reinterpret_cast<const Write *>(b + at.tab);
  const CAS uint32_t *pk0 = (const CAS uint32_t *)reinterpret_cast<const uint32_t *>(b + at.pk0);
  if (csum)
    hipLaunchKernelGGL(frame_fused_gather_batch_kernel<true>, dim3(groups), dim3(64 * kWaves),
                       (crc::kImageWords + kHdrWords) * sizeof(uint32_t), stream, ft, wt, pk0, nw, total_pk, proto,
                       crc_tab);
  else
    hipLaunchKernelGGL(frame_fused_gather_batch_kernel<false>, dim3(groups), dim3(64 * kWaves),
                       kHdrWords * sizeof(uint32_t), stream, ft, wt, pk0, nw, total_pk, proto, crc_tab);
  return hipGetLastError();
}

}  // namespace hdfs_wirev_fused_batch
