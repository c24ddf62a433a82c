// Host side shared by libhadoofus_writev.so (writev.cpp) and
// libhadoofus_wirev.so (wirev.cpp) only: how a write held in fragments is
// split between in-place segments and gathered chunks (Layout, build_layout),
// the slicing tables of gather_chunks_kernel, and the run that leaves the
// write's chunk CRCs in a device array (gather_plan, enqueue_gather).  One
// definition, included by both; each library compiles writev_kernels.hip for
// itself.  The including source brings the companions' host support (fail,
// engine_fail, DeviceBuffer) in ahead of this header.
#ifndef HADOOFUS_WRITEV_LAYOUT_H
#define HADOOFUS_WRITEV_LAYOUT_H

#ifndef HADOOFUS_COMPANION_SUPPORT_H
#error "include the companions' host support header first"
#endif

#include <algorithm>
#include <cstring>
#include <vector>

#include "crc32c_outpkt.h"
#include "crc32c_tables.h"
#include "hadoofus_writev.h"
#include "writev_internal.h"

namespace hdfs_writev {

using namespace hdfs_companion;

// A run of whole chunks inside one fragment shorter than this is not worth a
// segment-table entry: its chunks join the gathered set.  8 chunks are one
// tile of the main library's tiled kernel; a shorter run would be a ragged
// tile there, filled to less than its width, for the price of a table entry.
constexpr uint32_t kMinSegChunks = 8;

// ---- layout -----------------------------------------------------------------
// A run of whole chunks [chunk0, chunk0 + ...) inside fragment `frag`.
struct Run {
  int frag;
  uint64_t at;      // byte offset of the run in the fragment
  uint64_t len;     // bytes (the write's partial last chunk included)
  uint64_t chunk0;  // first chunk: its place in the CRC array
  uint64_t chunk1;  // one past the last
};

struct Layout {
  hdfs_writev_layout_info info;
  uint64_t n0 = 0;  // bytes of the short first chunk (0: the write starts on the grid)
  std::vector<Run> runs;
  std::vector<GChunk> chunks;  // filled only when bases are given
  std::vector<Piece> pieces;
};

// The chunk grid is hdfs_crc32c_compose_packets': a short first chunk that
// completes the block offset's chunk, then 512-B chunks, the last one possibly
// partial.  bases == NULL: counts only.
inline int build_layout(const uint64_t *lens, const void *const *bases, int n, int64_t off, Layout &L) {
  using hdfs_crc32c::outpkt::kWriteChunk;
  L = Layout{};
  hdfs_writev_layout_info &I = L.info;
  std::memset(&I, 0, sizeof(I));
  I.min_seg_chunks = kMinSegChunks;
  uint64_t total = 0;
  for (int f = 0; f < n; f++) {
    if (lens[f] > (uint64_t(1) << 62) - total) return fail(HDFS_CRC32C_EINVAL, "fragment %d: the write's length overflows", f);
    total += lens[f];
  }
  const uint64_t cs = kWriteChunk;
  const uint64_t n0 = (total && off % int64_t(cs)) ? std::min<uint64_t>(total, cs - uint64_t(off % int64_t(cs))) : 0;
  const uint64_t k0 = n0 ? 1 : 0;
  const uint64_t nchunks = k0 + (total - n0 + cs - 1) / cs;
  if (nchunks > 0xFFFFFFF0ull) return fail(HDFS_CRC32C_EINVAL, "more than 2^32 - 16 chunks in one write");
  L.n0 = n0;
  I.total = total;
  I.nchunks = nchunks;
  auto start = [&](uint64_t i) { return i < k0 ? 0 : n0 + (i - k0) * cs; };
  auto end = [&](uint64_t i) { return std::min(start(i + 1), total); };
  // runs of grid chunks wholly inside one fragment
  uint64_t a = 0;
  for (int f = 0; f < n; f++) {
    if (!lens[f]) continue;
    const uint64_t b = a + lens[f];
    const uint64_t i0 = a <= n0 ? k0 : k0 + (a - n0 + cs - 1) / cs;               // first grid chunk starting at or after a
    const uint64_t i1 = b == total ? nchunks : (b < n0 ? 0 : k0 + (b - n0) / cs);  // chunks ending at or before b
    if (i1 > i0 && i1 - i0 >= kMinSegChunks) {
      L.runs.push_back(Run{f, start(i0) - a, end(i1 - 1) - start(i0), i0, i1});
      I.nsegments++;
      I.seg_chunks += i1 - i0;
    }
    a = b;
  }
  // every other chunk is gathered from its pieces
  I.ngathered = nchunks - I.seg_chunks;
  if (bases) L.chunks.reserve(size_t(I.ngathered));
  int f = 0;        // the first fragment that may reach into the chunk at hand
  uint64_t fa = 0;  // its offset in the write
  size_t ri = 0;
  for (uint64_t i = 0; i < nchunks; i++) {
    if (ri < L.runs.size() && i == L.runs[ri].chunk0) {
      i = L.runs[ri++].chunk1 - 1;
      continue;
    }
    const uint64_t s = start(i), e = end(i);
    while (fa + lens[f] <= s) fa += lens[f++];  // s < total: ends inside the list
    uint64_t pos = s, ga = fa;
    uint32_t count = 0;
    for (int g = f; pos < e; g++) {
      const uint64_t ge = ga + lens[g];
      if (ge > pos) {  // (a zero-length fragment has no piece)
        const uint64_t take = std::min(e, ge) - pos;
        if (bases) L.pieces.push_back(Piece{static_cast<const uint8_t *>(bases[g]) + (pos - ga), uint32_t(take), 0u});
        pos += take;
        count++;
      }
      ga = ge;
    }
    if (I.npieces + count > 0xFFFFFFF0ull) return fail(HDFS_CRC32C_EINVAL, "more than 2^32 - 16 pieces in one write");
    if (bases) L.chunks.push_back(GChunk{uint32_t(i), uint32_t(I.npieces), count, 0u});
    I.npieces += count;
    I.max_pieces = std::max(I.max_pieces, count);
  }
  return HDFS_CRC32C_OK;
}

// ---- the slicing tables ---------------------------------------------------------
// *slice <- a device u32[2][kSliceWords] on the current device: the tables of
// CRC32C, then those of CRC32.  On failure *slice is NULL.
inline hipError_t upload_slicing_tables(uint32_t **slice) {
  hipError_t e = hipMalloc(slice, 2 * kSliceWords * sizeof(uint32_t));
  if (e != hipSuccess) *slice = nullptr;
  if (e == hipSuccess) {
    std::vector<uint32_t> t(2 * kSliceWords);
    hdfs_crc32c::make_slicing4(reinterpret_cast<uint32_t(*)[256]>(t.data()), hdfs_crc32c::kPoly);
    hdfs_crc32c::make_slicing4(reinterpret_cast<uint32_t(*)[256]>(t.data() + kSliceWords), hdfs_crc32c::kPolyZlib);
    e = hipMemcpy(*slice, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(*slice);
      *slice = nullptr;
    }
  }
  return e;
}

// ---- the CRCs of a gather write ----------------------------------------------------
// Bytes of the device tables of layout L: the gathered chunks, then their pieces.
inline size_t gather_table_bytes(const Layout &L) {
  return size_t(L.info.ngathered) * sizeof(GChunk) + size_t(L.info.npieces) * sizeof(Piece);
}

// In place: every run is one segment of one compute plan, its CRCs at the
// run's place in the write's CRC array d_crc.  *cplan stays NULL when the
// write has no run.  Enqueues nothing.
inline int gather_plan(const hdfs_crc32c_iovec *iov, const Layout &L, int ctype, uint32_t *d_crc,
                       hdfs_crc32c_plan **cplan) {
  using hdfs_crc32c::outpkt::kWriteChunk;
  *cplan = nullptr;
  if (L.runs.empty()) return HDFS_CRC32C_OK;
  const bool zlib = ctype == HDFS_CRC32C_CSUM_CRC32;
  std::vector<hdfs_crc32c_segment> segs(L.runs.size());
  for (size_t i = 0; i < segs.size(); i++) {
    const Run &r = L.runs[i];
    segs[i] = hdfs_crc32c_segment{static_cast<const uint8_t *>(iov[r.frag].base) + r.at, r.len, kWriteChunk,
                                  HDFS_CRC32C_SEG_BE | (zlib ? HDFS_CRC32C_SEG_CRC32 : 0u), 0u, 0u,
                                  d_crc + r.chunk0, nullptr};
  }
  const int rc = hdfs_crc32c_plan_create(cplan, HDFS_CRC32C_MODE_COMPUTE, segs.data(), segs.size());
  return rc ? engine_fail(rc, "compute plan") : rc;
}

// On stream st: the tables of L to d_tab (gather_table_bytes(L) of room), the
// plan (may be NULL) over the runs, then gather_chunks_kernel over the rest:
// afterwards d_crc[i] is chunk i's CRC in wire byte order.  slice:
// upload_slicing_tables'.  -> the engine's status; *e: the runtime's.  The
// caller synchronises st before L or the tables go, whatever the two say.
inline int enqueue_gather(const Layout &L, hdfs_crc32c_plan *cplan, int ctype, void *d_tab, const uint32_t *slice,
                          uint32_t *d_crc, hipStream_t st, hipError_t *e) {
  const hdfs_writev_layout_info &I = L.info;
  const size_t ch_bytes = size_t(I.ngathered) * sizeof(GChunk), pc_bytes = size_t(I.npieces) * sizeof(Piece);
  GChunk *d_ch = static_cast<GChunk *>(d_tab);
  Piece *d_pc = reinterpret_cast<Piece *>(static_cast<uint8_t *>(d_tab) + ch_bytes);
  const bool zlib = ctype == HDFS_CRC32C_CSUM_CRC32;
  int rc = HDFS_CRC32C_OK;
  *e = hipSuccess;
  if (ch_bytes) *e = hipMemcpyAsync(d_ch, L.chunks.data(), ch_bytes, hipMemcpyHostToDevice, st);
  if (*e == hipSuccess && pc_bytes) *e = hipMemcpyAsync(d_pc, L.pieces.data(), pc_bytes, hipMemcpyHostToDevice, st);
  if (*e == hipSuccess && cplan && (rc = hdfs_crc32c_plan_execute(cplan, st))) rc = engine_fail(rc, "compute plan");
  if (*e == hipSuccess && !rc)
    *e = launch_gather_chunks(d_ch, uint32_t(I.ngathered), d_pc, uint32_t(I.npieces), slice + (zlib ? kSliceWords : 0),
                              d_crc, uint32_t(I.nchunks), st);
  return rc;
}

}  // namespace hdfs_writev

#endif  // HADOOFUS_WRITEV_LAYOUT_H
