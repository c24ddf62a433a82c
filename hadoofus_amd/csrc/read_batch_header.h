// The header comparison of a packet on the read side, for
// unframe_scatter_batch_kernel (preadv_batch_kernels.hip).  Device code; hipcc
// only.  read_batch_kernels.hip and pread_batch_kernels.hip each hold this
// function's text themselves, because their CPU tests keep that text where it
// is; it stands here in a header of its own so that a later change can fold
// those two into it.
#ifndef HADOOFUS_READ_BATCH_HEADER_H
#define HADOOFUS_READ_BATCH_HEADER_H

#include "crc32c_outpkt.h"
#include "read_batch_layout.h"
#include "read_batch_verify.h"

namespace hdfs_read_batch {

// The packet's header, by one whole wave: lane 0 composes the expected one
// into LDS (hdr: 16 words, 33 bytes at most), lane t compares byte t with the
// stream's.
FUSED_DEV bool verify_header(uint32_t *hdr, uint32_t proto, const Round &r, uint32_t lane) {
  const Unit &u = r.u;
  if (lane == 0u) {
    uint8_t *p = reinterpret_cast<uint8_t *>(hdr);
    uint8_t *e = hdfs_crc32c::outpkt::put_out_header(p, int(proto), u.p.off, u.p.seq, u.p.last != 0u,
                                                     int32_t(u.p.dlen), u.p.ncrc);
    if (has_sync(int(proto), u.hb)) {  // hlen 27: syncBlock behind the required fields
      p[5] = uint8_t(hdfs_crc32c::outpkt::kHdrProtoBytes + 2u);
      e[0] = 0x28;
      e[1] = r.sync ? 1 : 0;
    }
  }
  // a wave's LDS operations execute in order; the fences keep the compiler from reordering them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const uint32_t want = reinterpret_cast<const uint8_t *>(hdr)[lane];
  const uint32_t got = load8(range_of(u.h0, u.hb), lane) & 0xFFu;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  return lane < u.hb && got != want;
}

}  // namespace hdfs_read_batch

#endif  // HADOOFUS_READ_BATCH_HEADER_H
