// Host side shared by the batch libraries (wire_batch.cpp,
// wire_fused_batch.cpp, wirev_fused_batch.cpp): everything a batch call does
// before it takes its lock.  The layout of every entry and the totals, the
// records, the argument checks of a call that has stream buffers and where
// those buffers lie.  One definition, included by all, templated on the entry
// struct (the first two libraries' public ones are field for field the same;
// the gather batch library lays out a private entry of that shape whose len is
// the sum of a write's fragments and checks its fragments' places itself).
// Each library keeps its own limits and the order in which it judges them.  No
// kernel file includes it.
#ifndef HADOOFUS_WIRE_BATCH_LAYOUT_H
#define HADOOFUS_WIRE_BATCH_LAYOUT_H

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

#include "wire_layout.h"

namespace hdfs_wire {

// What this file assumes of an entry struct: hdfs_wire_batch_write's layout.
template <class Entry>
constexpr bool entry_layout_ok() {
  static_assert(std::is_standard_layout<Entry>::value && sizeof(Entry) == 80, "the public entry struct");
  static_assert(offsetof(Entry, data) == 0 && offsetof(Entry, len) == 8 && offsetof(Entry, offset_in_block) == 16 &&
                    offsetof(Entry, seqno) == 24 && offsetof(Entry, finish) == 32 && offsetof(Entry, wire) == 40 &&
                    offsetof(Entry, wire_cap) == 48,
                "the public entry struct: in");
  static_assert(offsetof(Entry, wire_len) == 56 && offsetof(Entry, npkts) == 64 && offsetof(Entry, first_pkt) == 72,
                "the public entry struct: out");
  static_assert(std::is_same<decltype(Entry::len), uint64_t>::value &&
                    std::is_same<decltype(Entry::offset_in_block), int64_t>::value &&
                    std::is_same<decltype(Entry::finish), int32_t>::value &&
                    std::is_same<decltype(Entry::first_pkt), uint64_t>::value,
                "the public entry struct: types");
  return true;
}

// An entry of either library's device table.  tests/test_gpu_companion_scratch.py
// counts on the size when it walks a batch's table across kTableFloor.
static_assert(sizeof(Write) == 80, "the device table's entry");

// The failure just recorded (by the shared layout code) was entry k's.
inline int entry_fail(int rc, size_t k) { return prefix_fail(rc, "entry %zu", k); }

// ---- layout of the batch ------------------------------------------------------------
struct Batch {
  std::vector<Layout> L;  // per entry
  uint64_t npkts = 0, nchunks = 0, wire_bytes = 0, entries = 0;
};

// The batch's chunks and packets in closed form.
struct Counts {
  uint64_t chunks = 0, packets = 0;
};

// The list itself and every entry's arguments are judged, every entry's out
// fields are zeroed and the totals are counted in closed form: a library
// refuses a batch past its limit before any write's packets are walked.
template <class Entry>
int count_batch(Entry *w, size_t n, int max_writes, int proto, int ctype, Counts &c) {
  static_assert(entry_layout_ok<Entry>(), "");
  if (n > size_t(max_writes)) return fail(HDFS_CRC32C_EINVAL, "%zu writes, at most %d in one call", n, max_writes);
  if (n && !w) return fail(HDFS_CRC32C_EINVAL, "null writes");
  for (size_t k = 0; k < n; k++) w[k].wire_len = w[k].npkts = w[k].first_pkt = 0;
  for (size_t k = 0; k < n; k++) {
    if (!args_ok(proto, ctype, w[k].offset_in_block, w[k].len)) return entry_fail(HDFS_CRC32C_EINVAL, k);
    const uint64_t mis = uint64_t(w[k].offset_in_block) % kChunk, to_grid = mis ? kChunk - mis : 0u;
    const uint64_t n0 = std::min(w[k].len, to_grid), rest = w[k].len - n0;
    c.chunks += (n0 ? 1u : 0u) + (rest + kChunk - 1) / kChunk;  // <= 2^31 + 1 each, 65 536 of them
    c.packets += (n0 ? 1u : 0u) + (rest + kPacket - 1) / kPacket + (w[k].finish ? 1u : 0u);
  }
  return HDFS_CRC32C_OK;
}

// Walks every write's packets: fills the out fields of every entry and the
// totals.  The caller judges the totals afterwards, so every entry's out
// fields are set by then.
template <class Entry>
int layout_entries(Entry *w, size_t n, int proto, int ctype, Batch &B) {
  B.L.resize(n);
  for (size_t k = 0; k < n; k++) {
    Layout &L = B.L[k];
    const int rc = build_layout(w[k].len, w[k].offset_in_block, w[k].seqno, proto, ctype, w[k].finish != 0, L);
    if (rc) return entry_fail(rc, k);
    w[k].wire_len = L.wire_len;
    w[k].npkts = L.plan.size();
    w[k].first_pkt = B.npkts;
    B.npkts += L.plan.size();
    B.nchunks += L.nchunks;
    B.wire_bytes += L.wire_len;
    B.entries += L.plan.empty() ? 0u : 1u;
  }
  return HDFS_CRC32C_OK;
}

// The body of a library's _layout entry point; layout(B) is its layout_batch.
template <class Totals, class LayoutBatch>
int layout_totals(Totals *out, LayoutBatch layout) {
  if (!out) return fail(HDFS_CRC32C_EINVAL, "null out");
  std::memset(out, 0, sizeof(*out));
  Batch B;
  const int rc = layout(B);
  out->npkts = B.npkts;
  out->nchunks = B.nchunks;
  out->wire_bytes = B.wire_bytes;
  out->table_entries = B.entries;
  return rc;
}

template <class Entry>
void fill_batch_records(const Entry *w, const Batch &B, hdfs_crc32c_out_packet *pkts) {
  for (size_t k = 0; k < B.L.size(); k++) fill_records(B.L[k], pkts + w[k].first_pkt);
}

// ---- the arguments of a call that has stream buffers ----------------------------------
// Entries whose wire is set: none is a size query.
template <class Entry>
size_t count_wires(const Entry *w, size_t n) {
  size_t with_wire = 0;
  for (size_t k = 0; k < n; k++) with_wire += w[k].wire ? 1u : 0u;
  return with_wire;
}

// with_wire > 0 of the n entries have a stream buffer: all of them must, with
// room for their stream and their records, and data where there are bytes.
template <class Entry>
int check_entries(const Entry *w, size_t n, size_t with_wire, const Batch &B, const hdfs_crc32c_out_packet *pkts,
                  size_t max_pkts) {
  if (with_wire != n) {
    const bool first = w[0].wire != nullptr;
    size_t k = 1;
    while ((w[k].wire != nullptr) == first) k++;
    return fail(HDFS_CRC32C_EINVAL, "entry %zu: wire is %s, entry 0's is not (every wire NULL is a size query)", k,
                first ? "NULL" : "set");
  }
  for (size_t k = 0; k < n; k++) {
    if (w[k].len && !w[k].data)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: null data with %llu bytes", k, (unsigned long long)w[k].len);
    if (w[k].wire_cap < w[k].wire_len)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: %llu stream bytes, room for %llu", k,
                  (unsigned long long)w[k].wire_len, (unsigned long long)w[k].wire_cap);
    if (pkts && w[k].first_pkt + w[k].npkts > max_pkts)
      return fail(HDFS_CRC32C_EINVAL, "entry %zu: its records end at %llu of %llu, room for %zu", k,
                  (unsigned long long)(w[k].first_pkt + w[k].npkts), (unsigned long long)B.npkts, max_pkts);
  }
  return HDFS_CRC32C_OK;
}

// ---- where the buffers live -------------------------------------------------------
// No wire range overlaps another wire range or a data range: the sweep of the
// companions' shared host support (hdfs_companion::check_overlaps, which the
// read-side libraries call too), with its default nouns "wire" and "data".
using hdfs_companion::check_overlaps;
using hdfs_companion::Span;
using hdfs_companion::span_before;

// Every entry's data and stream inside one allocation of device `dev` each,
// and no stream over another stream or over any data.
template <class Entry>
int check_batch_places(const Entry *w, size_t n, int dev) {
  int rc;
  Allocations al;
  std::vector<Span> spans;
  spans.reserve(2 * n);
  for (size_t k = 0; k < n; k++) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(w[k].data), b = reinterpret_cast<uintptr_t>(w[k].wire);
    if (w[k].len) {
      if ((rc = al.check(w[k].data, w[k].len, dev, "data"))) return entry_fail(rc, k);
      spans.push_back(Span{a, a + uintptr_t(w[k].len), uint32_t(k), 0u});
    }
    if (w[k].wire_len) {
      if ((rc = al.check(w[k].wire, w[k].wire_len, dev, "wire"))) return entry_fail(rc, k);
      spans.push_back(Span{b, b + uintptr_t(w[k].wire_len), uint32_t(k), 1u});
    }
  }
  return check_overlaps(spans);
}

}  // namespace hdfs_wire

#endif  // HADOOFUS_WIRE_BATCH_LAYOUT_H
