// site_map.hpp -- the sparse mode of the per-site table (dyn_aligner_set_site_summary_sparse): an open-addressing hash map on
// the device from a site id to a row of a table with `capacity` rows. Inline functions only, no kernels: any number of
// translation units may include this file (site_summary_kernels.hpp looks rows up while it fills, site_map_kernels.hpp gathers
// and scatters windows of ids, tests/device_math/site_map.hip exports sm_home to the tests).
//
// Definition. keys[capacity] uint32, SM_EMPTY = 0xFFFFFFFF = DYN_SITE_NONE (never a valid id: one
// memset to 0xFF empties the map). The bucket index IS the table row. The home bucket of an id is a multiplicative hash reduced
// by multiply-shift, so any capacity >= 1 works:
//   sm_home(id, capacity) = ((uint32)(id * 0x9E3779B1) * (uint64)capacity) >> 32
// Probing is linear with wrap-around over at most min(capacity, SM_PROBE_MAX) buckets: a cap on the work of a row that a full
// map drops, not a tuned value.
// Nothing is ever deleted and a key, once written, never changes: a probe window that is full stays full. A key is therefore
// either in the map with ALL of its rows or absent with all of them dropped, whatever the order of the atomics. No thread waits
// for another one and no second word is published: the cells behind a bucket are zeroed at allocation and only ever touched by
// atomics, so a row may add to its cell the moment its compare-and-swap (or its load) shows the key.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nt_kernels.hpp"

namespace dynk {

constexpr uint32_t SM_EMPTY = 0xFFFFFFFFu;
constexpr uint32_t SM_NO_ROW = 0xFFFFFFFFu;  // what a lookup returns for "absent" / "no bucket" (a row is < capacity <= 2^32 - 1)
constexpr uint32_t SM_PROBE_MAX = 128;
constexpr uint32_t SM_HASH_MUL = 0x9E3779B1u;  // 2^32 / the golden ratio, odd
// (the [3] statistics beside the table, SM_N_KEYS / SM_ROWS_DROPPED / SM_SITES_DROPPED: nt_kernels.hpp)

__host__ __device__ inline uint32_t sm_home(uint32_t id, uint32_t capacity) {
  return (uint32_t)(((uint64_t)(uint32_t)(id * SM_HASH_MUL) * (uint64_t)capacity) >> 32);
}

__device__ __forceinline__ uint32_t sm_load_key(const uint32_t* keys, uint32_t h) {
  return __hip_atomic_load(keys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the row of id, or SM_NO_ROW: stops at the key, at an empty bucket or at the end of the probe window; never writes
__device__ __forceinline__ uint32_t sm_find(const uint32_t* keys, uint32_t capacity, uint32_t id) {
  uint32_t h = sm_home(id, capacity);
  const uint32_t n = capacity < SM_PROBE_MAX ? capacity : SM_PROBE_MAX;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t k = sm_load_key(keys, h);
    if (k == id) return h;
    if (k == SM_EMPTY) return SM_NO_ROW;
    h = h + 1u == capacity ? 0u : h + 1u;
  }
  return SM_NO_ROW;
}

// the row of id, inserted when absent; SM_NO_ROW when the probe window holds other keys only. The compare-and-swap runs only on
// a bucket seen empty; the thread whose swap took the bucket counts the key.
__device__ __forceinline__ uint32_t sm_find_or_insert(uint32_t* keys, uint32_t capacity, unsigned long long* stats, uint32_t id) {
  uint32_t h = sm_home(id, capacity);
  const uint32_t n = capacity < SM_PROBE_MAX ? capacity : SM_PROBE_MAX;
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t k = sm_load_key(keys, h);
    if (k == SM_EMPTY) {
      k = atomicCAS(keys + h, SM_EMPTY, id);
      if (k == SM_EMPTY) {
        atomicAdd(stats + SM_N_KEYS, 1ull);
        return h;
      }
    }
    if (k == id) return h;
    h = h + 1u == capacity ? 0u : h + 1u;
  }
  return SM_NO_ROW;
}

}  // namespace dynk
