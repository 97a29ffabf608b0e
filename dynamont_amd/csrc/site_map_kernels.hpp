// site_map_kernels.hpp -- the window calls of a sparse per-site table (site_map.hpp): a window of ids gathered into a dense scratch
// that the existing window kernels (quantiles, compare, mixture) and copies read unchanged, the exact add of host columns
// scattered into the rows of a window of ids, and the bitmap of the id windows that hold a key. Included by site_summary.hip
// (launch_site_gather, launch_site_scatter_add, launch_site_map_windows) and by tests/device_math/site_map.hip. The kernels are
// ordinary (non-inline) definitions: one translation unit per binary includes this file.
//
// SMK_LANES = 16 consecutive lanes serve one site, so that the loads and stores of a row's words coalesce: every lane of the group
// looks the id up (the same addresses: one request), then lane f < 7 moves field f and the lanes stride over the counters.
// Footprint: 256 threads, no LDS, no scratch.
#pragma once
#define DYNK_SITE_MAP_KERNELS_HPP 1  // (site_pack_kernels.hpp asks for this header in front of it)

#include "exact_sum_kernels.hpp"
#include "nt_kernels.hpp"
#include "site_map.hpp"

namespace dynk {

constexpr int SMK_LANES = 16;
constexpr int SMK_SITES_PER_BLOCK = 256 / SMK_LANES;

// 64-bit and 32-bit words of a cell that a filling kernel may be adding to: one relaxed device-scope load each, never torn
__device__ __forceinline__ unsigned long long smk_load64(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned int smk_load32(const unsigned int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid ceil(count / 16): lanes [16 g, 16 g + 16) of a block own site blockIdx.x * 16 + g of the window
__global__ __launch_bounds__(256) void k_site_gather(SiteGather sg) {
  const uint32_t t = blockIdx.x * (uint32_t)SMK_SITES_PER_BLOCK + threadIdx.x / SMK_LANES;
  const uint32_t lane = threadIdx.x % SMK_LANES;
  if (t >= sg.count) return;
  const uint32_t row = sm_find(sg.keys, sg.capacity, sg.lo + t);  // (lo + count <= num_sites < 2^32: no wrap)
  if (sg.out_acc && lane < (uint32_t)SS_FIELDS)
    sg.out_acc[(uint64_t)t * SS_FIELDS + lane] = row == SM_NO_ROW ? 0ull : smk_load64(sg.acc + (uint64_t)row * SS_FIELDS + lane);
  if (sg.hist) {
    const unsigned int* src = sg.hist + (uint64_t)row * sg.width;
    unsigned int* dst = sg.out_hist + (uint64_t)t * sg.width;
    for (uint32_t w = lane; w < sg.width; w += SMK_LANES) dst[w] = row == SM_NO_ROW ? 0u : smk_load32(src + w);
  }
}

inline void launch_site_gather_kernel(const SiteGather& sg, hipStream_t s) {
  if (!sg.keys || !sg.capacity || !sg.acc || sg.count == 0 || (!sg.out_acc && !sg.hist) || (sg.hist && (!sg.out_hist || sg.width == 0))) return;
  const unsigned blocks = (sg.count + SMK_SITES_PER_BLOCK - 1) / SMK_SITES_PER_BLOCK;
  hipLaunchKernelGGL(k_site_gather, dim3(blocks), dim3(256), 0, s, sg);
}

// grid ceil(count / 16), the groups as above. The group ORs the site's staged words; when any is set its lane 0 finds or inserts
// the id and hands the row to the others, which then add exactly what k_site_add adds: fields 0 .. 2 by 64-bit atomic adds, M1 and
// M2 through xs_add128, the counters by 32-bit atomic adds, a zero never sent. Thread 0 of the grid adds the caller's totals.
__global__ __launch_bounds__(256) void k_site_scatter_add(SiteScatter sc) {
  const uint32_t t = blockIdx.x * (uint32_t)SMK_SITES_PER_BLOCK + threadIdx.x / SMK_LANES;
  const uint32_t lane = threadIdx.x % SMK_LANES;
  const bool live = t < sc.count;  // (no early return: the whole group takes part in the shuffles below)
  const unsigned long long* __restrict__ src = sc.cols + (uint64_t)t * SS_FIELDS;
  const unsigned int* __restrict__ cnt = sc.counters + (uint64_t)t * sc.width;
  unsigned int any = 0;
  if (live) {
    if (lane < (uint32_t)SS_FIELDS) any = src[lane] != 0ull;
    if (sc.hist)
      for (uint32_t w = lane; w < sc.width; w += SMK_LANES) any |= cnt[w] != 0u;
  }
  for (int d = SMK_LANES >> 1; d > 0; d >>= 1) any |= (unsigned int)__shfl_xor((int)any, d, SMK_LANES);
  uint32_t row = SM_NO_ROW;
  if (any && lane == 0) {
    row = sm_find_or_insert(sc.keys, sc.capacity, sc.stats, sc.lo + t);
    if (row == SM_NO_ROW) atomicAdd(sc.stats + SM_SITES_DROPPED, 1ull);
  }
  row = (uint32_t)__shfl((int)row, 0, SMK_LANES);
  if (row != SM_NO_ROW) {
    unsigned long long* cell = sc.acc + (uint64_t)row * SS_FIELDS;
    if (lane < 3) {
      if (src[lane]) atomicAdd(cell + lane, src[lane]);
    } else if (lane == 3) {
      xs_add128(cell + 3, src[3], src[4]);
    } else if (lane == 4) {
      xs_add128(cell + 5, src[5], src[6]);
    }
    if (sc.hist) {
      unsigned int* h = sc.hist + (uint64_t)row * sc.width;
      for (uint32_t w = lane; w < sc.width; w += SMK_LANES) {
        const unsigned int v = cnt[w];
        if (v) atomicAdd(h + w, v);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && sc.add_totals)
    for (int f = 0; f < SS_TOTALS; ++f)
      if (sc.totals_in[f]) atomicAdd(sc.totals + f, sc.totals_in[f]);
}

inline void launch_site_scatter_add_kernel(const SiteScatter& sc, hipStream_t s) {
  if (!sc.keys || !sc.capacity || !sc.stats || !sc.acc || !sc.totals || !sc.cols || sc.count == 0 ||
      (sc.hist && (!sc.counters || sc.width == 0)))
    return;
  const unsigned blocks = (sc.count + SMK_SITES_PER_BLOCK - 1) / SMK_SITES_PER_BLOCK;
  hipLaunchKernelGGL(k_site_scatter_add, dim3(blocks), dim3(256), 0, s, sc);
}

// one thread per bucket
__global__ __launch_bounds__(256) void k_site_map_windows(SiteWindows sw) {
  const uint64_t b = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (b >= sw.capacity) return;
  const uint32_t k = sw.keys[b];
  if (k == SM_EMPTY) return;
  const uint32_t win = k >> sw.shift;
  atomicOr(sw.bitmap + (win >> 5), 1u << (win & 31u));
}

inline void launch_site_map_windows_kernel(const SiteWindows& sw, hipStream_t s) {
  if (!sw.keys || !sw.capacity || !sw.bitmap || sw.shift < 0 || sw.shift > 31) return;
  hipLaunchKernelGGL(k_site_map_windows, dim3((unsigned)(((uint64_t)sw.capacity + 255u) / 256u)), dim3(256), 0, s, sw);
}

}  // namespace dynk
