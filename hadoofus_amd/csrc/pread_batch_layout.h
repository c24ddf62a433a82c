// The window arithmetic of libhadoofus_pread_batch.so, written once for host
// and device: pread_probe_kernel (pread_batch_kernels.hip) runs it with one
// thread per entry on the streams in device memory, pread_batch.cpp
// synthesises the packet records from its result, and
// tests/consumer/pread_batch_selftest.cpp runs the same functions on
// host-built streams against a brute-force frame_step walk with
// frame::read_avail and the read loop's stop rules.  No HIP runtime call is
// made here.
//
// A positional read (hdfs_datanode_read(bloff, len), hdfs_crc32c_read_packets
// with read_len > 0) wants the block's bytes [client_offset, client_offset +
// read_len).  Its stream starts at a chunk boundary at or before
// client_offset, so packet 0 carries c_begin = client_offset - offsetInBlock
// bytes the caller did not ask for (frame::read_avail; 0 when the read starts
// at or before packet 0), and the read may stop short of the stream's end.
//
// The stream's shape is probe_entry's (read_batch_layout.h), called with the
// destination and the record array unbounded: K packets of dlen0 bytes, at
// most one shorter one, at most the empty last one.  Its data packets hold
// `payload` bytes; payload position x of the stream is the block's byte
// offsetInBlock(packet 0) + x.  The window is the payload range
//   [c_begin, w_end),  w_end = c_begin + read_len,
// and an entry is REGULAR when, beside probe_entry's verdict,
//   c_begin < dlen0 (signed difference; UNEXPECTED_READ_OFFSET otherwise),
//   w_end <= payload (the read completes inside the stream's data packets),
//   none of the first m - 1 packets carries lastPacketInBlock, m = the data
//     packets up to and including the one that holds payload byte w_end - 1,
//   every taken packet that probe_entry framed (packet K - 1, the shorter one)
//     names the offsetInBlock packet 0 predicts for it, so that read_avail
//     gives it c_begin 0 as it does the predicted body packets,
//   dst_cap >= read_len, and (records wanted) m <= max_pkts.
// For a regular entry the descriptor is cut to the m packets the read takes:
//   npk = m, consumed = the end of packet m - 1, delivered = read_len,
// later packets -- the empty last one included -- are neither read nor
// returned.  Payload byte x of [c_begin, w_end) goes to dst + (x - c_begin):
// every store lies in [dst, dst + read_len), read_len <= dst_cap.
#ifndef HADOOFUS_PREAD_BATCH_LAYOUT_H
#define HADOOFUS_PREAD_BATCH_LAYOUT_H

#include <stdint.h>

#include "crc32c_frame.h"
#include "read_batch_layout.h"

namespace hdfs_pread_batch {

using hdfs_read_batch::Desc;
using hdfs_read_batch::kChunk;
using hdfs_read_batch::kMaxEntries;
using hdfs_read_batch::kMaxPackets;
using hdfs_read_batch::kMaxTail;
using hdfs_read_batch::kNoSlot;
using hdfs_read_batch::packet_of;
using hdfs_read_batch::PacketAt;
using hdfs_read_batch::prefix_regular;
using hdfs_read_batch::probe_entry;
using hdfs_read_batch::record_of;

constexpr int64_t kMaxBlockOffset = int64_t(1) << 62;  // offsets and payloads above are not predicted

// One entry as uploaded.
struct Entry {
  const uint8_t *stream;
  uint64_t len;
  uint8_t *dst;
  uint64_t dst_cap;
  int64_t client_offset, read_len;
};

// What the probe leaves of a regular entry: the stream's descriptor cut to the
// packets the read takes (packet_of(d, i), i < d.npk; PacketAt::dst_off is the
// packet's payload position), and the window in payload positions.
struct Window {
  Desc d;
  uint64_t c_begin, w_end;
};

// Where packet p's delivered bytes come from and go: bytes [*from, *from +
// *n) of its data land at dst + *at.  What read_avail and read_place give the
// packets of a regular entry.
HDFS_HD void place_of(const Window &w, const PacketAt &p, uint32_t &from, uint64_t &at, uint32_t &n) {
  const uint64_t p0 = p.dst_off, p1 = p0 + p.dlen;
  const uint64_t a = p0 > w.c_begin ? p0 : w.c_begin, b = p1 < w.w_end ? p1 : w.w_end;
  from = uint32_t(a - p0);
  at = a - w.c_begin;
  n = b > a ? uint32_t(b - a) : 0u;
}

HDFS_HD void clear(Window &w) {
  Desc &d = w.d;
  d.stride = d.consumed = d.delivered = 0;
  d.off0 = d.seq0 = 0;
  d.dlen0 = d.hb0 = d.last0 = d.sync0 = d.nbody = d.ntail = d.npk = 0;
  w.c_begin = w.w_end = 0;
}

// at(pos): the stream's bytes from pos on, as probe_entry's.  Fills w but
// d.stream, d.dst and d.entry.  -> regular.
template <class At>
HDFS_HD bool probe_window(At at, uint64_t len, uint64_t dst_cap, int64_t client_offset, int64_t read_len, int proto,
                          uint32_t chunk_size, int ctype, bool want_records, uint64_t max_pkts, Window &w) {
  Desc &d = w.d;
  w.c_begin = w.w_end = 0;
  if (read_len <= 0 || client_offset < 0 ||
      !probe_entry(at, len, ~uint64_t(0), proto, chunk_size, ctype, false, 0, d)) {
    clear(w);
    return false;
  }
  const uint64_t payload = d.delivered, want = uint64_t(read_len);
  const uint64_t K = uint64_t(d.nbody) + 1u;  // packets of dlen0 bytes
  bool ok = d.off0 >= 0 && d.off0 <= kMaxBlockOffset && payload <= uint64_t(kMaxBlockOffset);
  uint64_t cb = 0;
  if (ok && d.off0 < client_offset) {  // frame::read_avail
    cb = uint64_t(client_offset) - uint64_t(d.off0);
    ok = cb < d.dlen0;
  }
  ok = ok && want <= payload && cb + want <= payload && want <= dst_cap;
  uint64_t m = 0;
  if (ok) {
    const uint64_t end = cb + want;
    m = end <= K * d.dlen0 ? (end + d.dlen0 - 1u) / d.dlen0 : K + 1u;  // the shorter packet completes it
    ok = m <= kMaxPackets && !(want_records && m > max_pkts);
    if (m > 1u && d.last0) ok = false;  // packet 0, and every body packet is predicted with its flags
    if (m == uint64_t(d.nbody) + 2u && d.tail[0].last) ok = false;  // packet K - 1 ahead of the shorter one
    // The tail is taken as framed, so its offsetInBlock is the stream's own: read_avail gives a later packet
    // c_begin 0 only when it lies where packet 0 predicts it (a body packet that does not is flagged by the
    // main launch's header comparison).  off0 and the payload are at most 2^62 each: no overflow.
    if (m > d.nbody && d.tail[0].off != d.off0 + int64_t(d.tail[0].dst_off)) ok = false;
    if (m == uint64_t(d.nbody) + 2u && d.tail[1].off != d.off0 + int64_t(d.tail[1].dst_off)) ok = false;
  }
  if (!ok) {
    clear(w);
    return false;
  }
  // cut to the m packets the read takes
  // (m <= nbody + 2; the tail is picked by comparison, not by a computed index: no private memory on the device)
  const PacketAt &end = m <= uint64_t(d.nbody) + 1u ? d.tail[0] : d.tail[1];
  const uint64_t consumed = m <= d.nbody  // a body packet's end, or the framed packet's
                                ? m * d.stride
                                : end.stream_off + end.hb + 4ull * hdfs_read_batch::crc_count(end.dlen) + end.dlen;
  const uint32_t nbody = d.nbody < m ? d.nbody : uint32_t(m);
  for (uint32_t t = 0; t < kMaxTail; t++)
    if (nbody + t >= m) d.tail[t] = PacketAt{0, 0, 0, 0, 0, 0, 0, 0};
  d.nbody = nbody;
  d.ntail = uint32_t(m) - nbody;
  d.npk = uint32_t(m);
  d.consumed = consumed;
  d.delivered = want;
  w.c_begin = cb;
  w.w_end = cb + want;
  return true;
}

}  // namespace hdfs_pread_batch

#endif  // HADOOFUS_PREAD_BATCH_LAYOUT_H
