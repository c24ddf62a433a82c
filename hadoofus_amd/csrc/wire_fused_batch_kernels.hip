// The wire streams of a batch of writes on gfx950 in ONE pass over the data
// and ONE launch: frame_fused_batch_kernel.
//
// The round is frame_fused_kernel's, the one definition of wire_fused_round.h:
// a workgroup is 16 waves, wave v takes round v (4 KiB, eight chunks) of the
// workgroup's current packet -- four coalesced 16-B buffer loads, the
// registers stored straight out (nt), the in-register transpose,
// wire_fused_crc.h's lane arithmetic, lane 8c's CRC store -- and wave 0
// composes and stores the header and does the chunk shorter than 512 B.  All
// bounds are by buffer descriptor, control flow is uniform, two register sets
// take turns, and the next packet's loads are issued ahead of the current
// round's stores.  The table image is filled once per workgroup, behind the
// only barrier.
//
// The unit differs.  Workgroup b walks global packets g = b, b + G, b + 2G,
// ... of the whole batch, counted in batch order (G workgroups, about one per
// CU).  For each g it finds the write k with pk0[k] <= g < pk0[k + 1]
// (write_of, wire_fused_batch_lookup.h: from the write found last, a bounded
// number of hops, then a bounded binary search) and takes packet g - pk0[k] of
// it.  g is uniform across the workgroup and the tables are read through the
// constant address space, as frame_batch_kernel reads them: the lookup and the
// load of the entry are scalar loads and a scalar loop.  The entry is live
// only inside unit_at; what the round needs of it is in the Unit, what holds
// for the whole batch (proto, csum) is a kernel argument.
//
// Writes without packets are dropped on the host (wire_fused_batch.cpp), so
// pk0 rises strictly and no entry with zero packets can be selected.  A g at
// or past the batch's last packet is a round of nothing: every range empty.
//
// Invariants.  Every byte of every [wire, wire + wire_len) is stored exactly
// once: the global packet indices tile the writes' packets, the packets tile
// each stream (wire_layout.h checks that on the host), and a packet's bytes
// are stored as frame_fused_kernel stores them.  No destination byte is read.
// No store falls outside a write's own stream, no load outside a write's
// [data, data + len).  No atomics, no cross-workgroup dependence, no spinning.
//
// hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S: 68 VGPRs, 106 SGPRs
// (52 / 90 without checksums), 159 776 B of dynamic LDS (32 B without),
// private_segment_fixed_size 0, no flat_ or scratch_ instruction; seven
// loop-invariant SGPRs live in VGPR lanes with checksums.  The waits the
// compiler chose are written up in DESIGN.md section 17.
#include "wire_fused_batch_internal.h"
#include "wire_fused_batch_lookup.h"
#include "wire_fused_round.h"

namespace hdfs_wire_fused {

#define CAS __attribute__((address_space(4)))

// The wave's round of global packet g; k: the write found last (a lower bound
// of this one), updated.  Everything is wave-uniform.
FUSED_DEV Unit unit_at(const CAS Write *tab, const CAS uint32_t *pk0, uint32_t nw, uint32_t total, uint32_t g,
                       uint32_t &k, uint32_t wave) {
  const bool in = g < total;
  if (in) k = write_of(pk0, nw, g, k);
  const CAS Write *p = tab + k;
  const Write w{p->data, p->crc, p->wire, p->len, p->off, p->seq, p->n0, p->npk, p->hb, p->proto, p->csum, p->finish,
                p->slices};
  return unit_of(w, in ? g - pk0[k] : w.npk, wave);  // i == npk: no packet
}

template <bool CSUM>
__global__ __launch_bounds__(1024) void frame_fused_batch_kernel(const CAS Write *wt, const CAS uint32_t *pk0,
                                                                 uint32_t nw, uint32_t total, uint32_t proto,
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
  uint32_t g = blockIdx.x, k = 0u;
  // Two register sets take turns, as in frame_fused_kernel.
  u32x4 ra[4], rb[4];
  Unit u = unit_at(wt, pk0, nw, total, g, k, wave);
  load_round(ra, u, lo);
  auto step = [&](const u32x4(&cur)[4], u32x4(&nxt)[4]) {
    const Unit un = unit_at(wt, pk0, nw, total, g + G, k, wave);  // g + G < 2^32: total < 2^29, G <= 1024
    load_round(nxt, un, lo);                                     // the next packet's loads, ahead of this round's stores
    store_round(cur, u, lo);
    crc_round<CSUM>(lds, cur, u, wave, lane, init512);
    if (wave == 0u) {
      header(hdr, proto, u, lane);
      ragged_chunk<CSUM>(lds, tab, u.src, u, lane);  // wave 0's round starts at the packet's first data byte
    }
    g += G;
    u = un;
  };
  while (g < total) {
    step(ra, rb);
    if (g >= total) break;
    step(rb, ra);
  }
}

hipError_t prepare_frame_fused_batch() {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&frame_fused_batch_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize,
                             int((crc::kImageWords + kHdrWords) * sizeof(uint32_t)));
}

hipError_t launch_frame_fused_batch(const void *tab, uint32_t nw, uint32_t total_pk, uint32_t proto, bool csum,
                                    const uint32_t *crc_tab, uint32_t groups, hipStream_t stream) {
  if (!total_pk) return hipSuccess;
  if (!tab || !nw || nw > total_pk || total_pk > 0x7FFFFFFFu / 4u || !groups || groups > kBatchMaxGroups ||
      (csum && !crc_tab))
    return hipErrorInvalidValue;
  const Write *t = static_cast<const Write *>(tab);
  const uint32_t *pk0 = reinterpret_cast<const uint32_t *>(t + nw);
  if (csum)
    hipLaunchKernelGGL(frame_fused_batch_kernel<true>, dim3(groups), dim3(64 * kWaves),
                       (crc::kImageWords + kHdrWords) * sizeof(uint32_t), stream, (const CAS Write *)t,
                       (const CAS uint32_t *)pk0, nw, total_pk, proto, crc_tab);
  else
    hipLaunchKernelGGL(frame_fused_batch_kernel<false>, dim3(groups), dim3(64 * kWaves), kHdrWords * sizeof(uint32_t),
                       stream, (const CAS Write *)t, (const CAS uint32_t *)pk0, nw, total_pk, proto, crc_tab);
  return hipGetLastError();
}

}  // namespace hdfs_wire_fused
