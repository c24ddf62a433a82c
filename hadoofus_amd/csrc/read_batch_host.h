// Host side shared by the six read-side libraries (read_batch.cpp,
// pread_batch.cpp, preadv_batch.cpp, relay_batch.cpp, crc_streams.cpp,
// md5crc_streams.cpp): the skeleton of a call whose probe kernel sorts the
// batch's entries into those the kernels take and those handed to the main
// library.  The run of the probe and the kernels with its timing loop, the
// collection of the entries' outcomes, the main library's read with unlimited
// record room, its packet walk in pieces, and the scratch of the libraries that
// run the fused round.  One definition, included by all; each library keeps its
// own entry struct, argument checks, tables and launches.  Nothing here calls
// an engine entry point unless a library instantiates it.  No kernel file
// includes it.
#ifndef HADOOFUS_READ_BATCH_HOST_H
#define HADOOFUS_READ_BATCH_HOST_H

#include <vector>

#include "companion_support.h"

namespace hdfs_companion {

// ---- the probed run -------------------------------------------------------------------
// A timing call's own arguments, judged before any device is asked.
inline int timing_args_ok(int iters, const double *ms_per_iter) {
  if (iters < 1 || !ms_per_iter) return fail(HDFS_CRC32C_EINVAL, "iters >= 1 and ms_per_iter are needed");
  return HDFS_CRC32C_OK;
}

// On stream st: bytes [up_off, up_off + up_bytes) of the pinned twin go up to
// the device table, launches() runs once (the probe and the kernels), and what
// they wrote, [back_off, bytes), comes back.  iters > 0: then launches() iters
// more times between the two events, and *ms_per_iter is one round's time.
// Always synchronised, even after an error: the tables are out of the device's
// use before the caller's lock goes.  A HIP error is "<what>: <text>".
template <class Launches>
int probed_run(hipStream_t st, const TablePair &tab, size_t up_off, size_t up_bytes, size_t back_off, size_t bytes,
               hipEvent_t *ev, int iters, double *ms_per_iter, const char *what, Launches launches) {
  uint8_t *pin = tab.pin.as<uint8_t>(), *dv = tab.dev.as<uint8_t>();
  hipError_t he = hipMemcpyAsync(dv + up_off, pin + up_off, up_bytes, hipMemcpyHostToDevice, st);
  if (he == hipSuccess) he = launches();
  if (he == hipSuccess) he = hipMemcpyAsync(pin + back_off, dv + back_off, bytes - back_off, hipMemcpyDeviceToHost, st);
  if (he == hipSuccess && iters) {
    he = hipEventRecord(ev[0], st);
    for (int i = 0; i < iters && he == hipSuccess; i++) he = launches();
    if (he == hipSuccess) he = hipEventRecord(ev[1], st);
  }
  const hipError_t se = hipStreamSynchronize(st);
  if (he == hipSuccess) he = se;
  float ms = 0;
  if (he == hipSuccess && iters && (he = hipEventElapsedTime(&ms, ev[0], ev[1])) == hipSuccess)
    *ms_per_iter = double(ms) / iters;
  return he == hipSuccess ? HDFS_CRC32C_OK : fail(HDFS_CRC32C_EHIP, "%s: %s", what, hipGetErrorString(he));
}

// ---- the entries' outcomes --------------------------------------------------------------
// Slot s of entry b names a descriptor of the probe's that names b back;
// entry_of(s) is read only where s is a descriptor.
template <class EntryOf>
bool slot_adds_up(uint32_t s, uint32_t no_slot, uint32_t nreg, size_t b, EntryOf entry_of) {
  return s == no_slot || (s < nreg && entry_of(s) == b);
}

inline int tables_fail(size_t b) {
  return fail(HDFS_CRC32C_EHIP, "internal: the probe's tables do not add up at entry %zu", b);
}

// The call's result out of its entries': the first failure (negative) with the
// text it left, however many entries failed after it; else the first packet
// error (positive); else 0.
struct Outcomes {
  int first_neg = 0, first_pos = 0;
  char neg_text[sizeof(g_err)] = "";
  void note(int r) {
    if (r < 0 && !first_neg) {
      first_neg = r;
      std::memcpy(neg_text, g_err, sizeof(neg_text));
    }
    if (r > 0 && !first_pos) first_pos = r;
  }
  int result() const {
    if (!first_neg) return first_pos;
    std::memcpy(g_err, neg_text, sizeof(neg_text));
    return first_neg;
  }
};

// ---- an entry handed to the main library: the read ------------------------------------------
// hdfs_crc32c_read_packets of one entry, exactly the call of the contract.
// own: the caller's record array for this entry (room for own_room), given to
// the one call as it is.  own == NULL: the walk must not be cut, so recs grows
// until it is not.  -> the engine's rc, its text untouched.
inline int read_unlimited(std::vector<hdfs_crc32c_packet> &recs, const void *stream, uint64_t len, int proto,
                          uint32_t chunk_size, int ctype, int64_t client_offset, int64_t read_len,
                          const hdfs_crc32c_iovec *iov, int iovcnt, hdfs_crc32c_packet *own, size_t own_room,
                          size_t *np, uint64_t *used, uint64_t *got) {
  if (own)
    return hdfs_crc32c_read_packets(stream, len, proto, chunk_size, ctype, client_offset, read_len, iov, iovcnt, own,
                                    own_room, np, used, got);
  // a complete framing-clean packet has at least 25 bytes, and one record ends the walk
  const uint64_t most = len / 25u + 2u;
  for (uint64_t room = most < 4096u ? most : 4096u;; room = room * 16u < most ? room * 16u : most) {
    if (recs.size() < room) recs.resize(size_t(room));
    const int rc = hdfs_crc32c_read_packets(stream, len, proto, chunk_size, ctype, client_offset, read_len, iov, iovcnt,
                                            recs.data(), size_t(room), np, used, got);
    if (rc < 0 || *np < room || room >= most) return rc;
  }
}

// ---- an entry handed to the main library: the walk --------------------------------------------
constexpr size_t kPieceRecords = 65536;  // records of one hdfs_crc32c_parse_packets call

struct Walk {
  uint64_t pos = 0, npkts = 0, payload = 0;  // stream bytes walked; records; bytes of the packets without an error
  int64_t offset_in_block = 0;               // of the first record
  int rc = 0;                                // < 0: the engine's failure, its text prefixed "entry <b>: parse_packets"
};

// hdfs_crc32c_parse_packets of entry b's stream with unlimited record room, in
// pieces of `piece` records: a piece that filled its room and ended neither in
// an error nor in the empty last packet goes on where it stopped.
// each(record, at): every record without an error, `at` the stream offset its
// piece started at.
template <class Each>
Walk walk_pieces(std::vector<hdfs_crc32c_packet> &recs, size_t piece, const uint8_t *s, uint64_t len, size_t b,
                 int proto, uint32_t chunk_size, int ctype, Each each) {
  Walk w;
  if (recs.size() < piece) recs.resize(piece);
  while (w.pos < len) {
    size_t np = 0;
    uint64_t used = 0;
    w.rc = hdfs_crc32c_parse_packets(s + w.pos, len - w.pos, proto, chunk_size, ctype, recs.data(), piece, &np, &used);
    if (w.rc < 0) {
      engine_fail(w.rc, "parse_packets");
      prefix_fail(w.rc, "entry %zu", b);
      return w;
    }
    for (size_t i = 0; i < np; i++) {
      const hdfs_crc32c_packet &k = recs[i];
      if (!w.npkts && !i) w.offset_in_block = k.offset_in_block;
      if (k.error) continue;
      w.payload += uint64_t(k.data_len);
      each(k, w.pos);
    }
    w.npkts += np;
    w.pos += used;
    const bool ended = np && recs[np - 1].data_len == 0;  // the empty last packet ends the walk
    if (w.rc || np < piece || ended || !used) break;
  }
  return w;
}

// ---- where the streams lie ---------------------------------------------------------------------
// Of a batch that writes nothing the caller names: every stream inside one
// allocation of device `dev`.
template <class Entry>
int check_stream_places(const Entry *e, size_t n, int dev) {
  Allocations al;
  for (size_t b = 0; b < n; b++) {
    if (!e[b].len) continue;
    const int rc = al.check(e[b].stream, e[b].len, dev, "stream");
    if (rc) return prefix_fail(rc, "entry %zu", b);
  }
  return HDFS_CRC32C_OK;
}

// ---- device state -----------------------------------------------------------------------------
// The scratch of a library that runs the fused round.  On the engine's device:
// the CRC tables and the workgroups of one launch (Fused: a
// hdfs_wire_fused::DeviceState over the library's prepare function), set up
// when the library is first used there and kept; the call's device tables and
// their pinned twin, grown on demand, never shrunk, kept between calls.  A
// library with further buffers derives from it and names them in release_more.
template <class Fused>
struct ReadScratch : DeviceScratch {
  Fused fused;
  TablePair tab;
  std::vector<hdfs_crc32c_packet> recs;  // a fallback entry's records when the caller wants none

  template <class ReleaseMore>
  int reserve(int to, size_t tab_bytes, ReleaseMore release_more) {
    int rc = bind(to, "stream", [&] {
      fused.release();
      tab.release();
      release_more();
    });
    if (rc || (rc = fused.setup(to))) return rc;
    return tab.reserve(tab_bytes, kTableFloor);
  }
  int reserve(int to, size_t tab_bytes) {
    return reserve(to, tab_bytes, [] {});
  }
};

}  // namespace hdfs_companion

#endif  // HADOOFUS_READ_BATCH_HOST_H
