// The comparisons of a round on the read side, shared by the two kernels that
// run the fused round backwards: unframe_fused_batch_kernel
// (read_batch_kernels.hip) and unframe_window_batch_kernel
// (pread_batch_kernels.hip).  Device code; hipcc only.  A round's loads and
// stores are wire_fused_round.h's; what is here turns its CRC store into a
// comparison with the stream's CRC bytes and reports a mismatch in the entry's
// status word.
#ifndef HADOOFUS_READ_BATCH_VERIFY_H
#define HADOOFUS_READ_BATCH_VERIFY_H

#include "wire_fused_round.h"

namespace hdfs_read_batch {

using namespace hdfs_wire_fused;  // the round: Unit, range_of, load_round, store_round, transpose, fold8, crc::

// The wave's round of a packet, and what the comparison needs beside it.
// u.h0, u.c0, u.d0: the packet's regions in the STREAM; u.src: the round's
// first byte there; u.dst: in the destination.
struct Round {
  Unit u;
  uintptr_t out0;    // the packet's first byte in the destination
  uintptr_t status;  // its entry's status word
  uint32_t sync;     // the header's syncBlock value, when it has one (u.hb above the canonical length)
};

FUSED_DEV uint32_t load32(__amdgpu_buffer_rsrc_t r, uint32_t o) {
  return __builtin_amdgcn_raw_buffer_load_b32(r, o, 0, 0);
}

// The wire bytes of the round's CRCs: lane 8c loads chunk c's (any byte
// address; the range is exactly the round's CRC words).
FUSED_DEV uint32_t load_crcs(const Unit &u, uint32_t wave, uint32_t lane) {
  const __amdgpu_buffer_rsrc_t r = range_of(u.c0 + 4u * uintptr_t(kRoundChunks * wave), 4u * u.nfr);
  return load32(r, (lane & 7u) == 0u ? 4u * (lane >> 3) : kNowhere);
}

// The lane saw something that is not what it expected: 1 into the entry's
// status word.  Issued by every lane (the others' offset is outside the range).
FUSED_DEV void flag(const Round &r, bool bad) {
  store32(range_of(r.status, 4u), bad ? 0u : kNowhere, 1u);
}

// The CRCs of the round's full chunks, from the registers of its loads,
// against the stream's: crc_round with the store turned into a comparison.
FUSED_DEV bool verify_round(const uint32_t *img, const u32x4 (&v)[4], uint32_t wire, const Unit &u, uint32_t lane,
                            uint32_t init512) {
  uint32_t val = 0u;
  if (u.nfr) {  // uniform; no vector-memory access inside
    uint32_t d[16];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      d[4 * k + 0] = v[k].x;
      d[4 * k + 1] = v[k].y;
      d[4 * k + 2] = v[k].z;
      d[4 * k + 3] = v[k].w;
    }
    transpose(d);
    val = crc::chunk_final(fold8(crc::piece_shift(img, lane & 7u, crc::piece_raw(img, lane, d))), init512);
  }
  return (lane & 7u) == 0u && (lane >> 3) < u.nfr && wire != val;
}

}  // namespace hdfs_read_batch

#endif  // HADOOFUS_READ_BATCH_VERIFY_H
