// Shared between wirev.cpp (host entry points) and wirev_kernels.hip.
#ifndef HADOOFUS_WIREV_INTERNAL_H
#define HADOOFUS_WIREV_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wire_internal.h"

namespace hdfs_wirev {

// One non-empty fragment of the write: its bytes lie at base, the first of
// them is byte `at` of the fragments' concatenation.  The table holds the nf
// fragments in order, `at` rising strictly from 0, and one sentinel behind
// them, {NULL, len}: fragment k is bytes [at[k], at[k + 1]) of the write.
struct Frag {
  const uint8_t *base;
  uint64_t at;
};
static_assert(sizeof(Frag) == 16, "Frag layout");

// Writes wire[0, wire_len) of write w (w.data unused: the data are the
// fragments'): w.npk * w.slices workgroups of 256.  tab: device Frag[nf + 1].
// sc1: the 16-B stores are write-through (a measurement; the product uses one
// policy, wirev.cpp).
hipError_t launch_frame_gather(const hdfs_wire::Write &w, const Frag *tab, uint32_t nf, bool sc1, hipStream_t stream);

}  // namespace hdfs_wirev

#endif  // HADOOFUS_WIREV_INTERNAL_H
