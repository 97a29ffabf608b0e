// site_pack_kernels.hpp -- the per-site table by content: the live rows of a window of table rows packed
// into (id, cells, counters) records, and such records added into a table by key. Included by site_summary.hip (launch_site_pack,
// launch_site_pack_write, launch_site_merge) and by tests/device_math/site_pack.hip. The kernels are ordinary (non-inline)
// definitions: one translation unit per binary includes this file.
//
// The conventions of site_map_kernels.hpp: SMK_LANES = 16 consecutive lanes serve one row, lane f < 7 moves field f and the lanes
// stride over the counters; a word that a filling kernel may be adding to is read with smk_load64 / smk_load32; 256 threads, no
// scratch. A wave is 64 lanes on this chip and __ballot returns 64 bits: the four groups of a wave vote at once.
//
// Pack. A row is LIVE iff its id lies in [site_lo, site_hi) and any of its 7 cell words or of its counters is non-zero (the id:
// the row of a dense table, the bucket's key of a sparse one -- an empty bucket has none, and a key alone makes no row live). A
// wave owns a CHUNK of SPK_CHUNK_ROWS = 64 consecutive rows and three passes run back to back on one stream:
//   k_site_pack_count   every wave ORs its rows' words, 4 rows a step, and stores the chunk's 64-bit live mask
//   k_site_pack_scan    one workgroup: the exclusive prefix sums of the masks' popcounts, SPK_SCAN_TILE chunks a step with a
//                       running carry, and the window's total
//   k_site_pack_write   every wave copies its live rows to record offset[chunk] + (the live rows in front within the chunk)
// so the records stand in ascending row order whatever the order the waves ran in, and two launches over the same table give the
// same bytes. The host reads the total between the scan and the write (to size the records), nothing else. A row that a filling
// kernel makes live between the passes is not packed, one packed is copied as it stands at the write: the call runs behind the
// quiescence of dyn_aligner_site_summary_fetch, where neither happens.
// The records of a window are three arrays of `total` entries: site uint32, cells [7] uint64, counters [width] uint32.
//
// Merge. 16 lanes per record. The group ORs the record's words; when any is set its lane 0 takes the row -- id + offset itself in
// a dense table, sm_find_or_insert of it in a sparse one -- and hands it to the others, which then add exactly what k_site_add
// adds: fields 0 .. 2 by 64-bit atomic adds, M1 and M2 through xs_add128, the counters by 32-bit atomic adds, a zero never sent.
// Records of one launch may name the same id: every add is an atomic. A record whose id finds no bucket is dropped WHOLE (the row
// is taken before any word is added) and counted in stats[SM_SITES_DROPPED]: the invariant of site_map.hpp holds. Thread 0 of the
// grid adds the caller's totals.
// Footprint: 256 threads, no scratch; the scan keeps 4 words of LDS.
#pragma once

// (SMK_LANES, SMK_SITES_PER_BLOCK, smk_load64 and smk_load32 are site_map_kernels.hpp's: a unit includes that header, which is
// to stay in one unit per binary, in front of this one)
#ifndef DYNK_SITE_MAP_KERNELS_HPP
#error "site_pack_kernels.hpp: include site_map_kernels.hpp first (SMK_LANES, smk_load64, smk_load32)"
#endif
#include "exact_sum_kernels.hpp"
#include "nt_kernels.hpp"
#include "site_map.hpp"

namespace dynk {

// (SPK_CHUNK_ROWS = 64, the rows of a wave, one bit each of its live mask: nt_kernels.hpp)
constexpr int SPK_CHUNKS_PER_BLOCK = 256 / 64;                // waves of a workgroup
constexpr int SPK_SCAN_PER_THREAD = 4;                        // consecutive chunks of a thread of the scan
constexpr int SPK_SCAN_TILE = 256 * SPK_SCAN_PER_THREAD;      // chunks of one step of the scan
constexpr int SPK_SCAN_TILE_ROWS = SPK_SCAN_TILE * SPK_CHUNK_ROWS;

// the id of table row `row`, or SM_EMPTY: an empty bucket, or an id outside the filter
__device__ __forceinline__ uint32_t spk_row_id(const SitePack& sp, uint64_t row) {
  const uint32_t id = sp.keys ? sm_load_key(sp.keys, (uint32_t)row) : (uint32_t)row;
  return (id != SM_EMPTY && id >= sp.site_lo && id < sp.site_hi) ? id : SM_EMPTY;
}

// grid ceil(chunks / 4): wave w of a block owns chunk blockIdx.x * 4 + w; group g of the wave looks at row 4 * step + g of it
__global__ __launch_bounds__(256) void k_site_pack_count(SitePack sp) {
  const uint32_t chunk = blockIdx.x * (uint32_t)SPK_CHUNKS_PER_BLOCK + threadIdx.x / 64u;
  const uint32_t wl = threadIdx.x % 64u, g = wl / SMK_LANES, lane = wl % SMK_LANES;
  if (chunk >= (sp.count + SPK_CHUNK_ROWS - 1) / SPK_CHUNK_ROWS) return;  // (the whole wave)
  unsigned long long mask = 0ull;
  for (uint32_t step = 0; step < SPK_CHUNK_ROWS / 4; ++step) {
    const uint32_t r = chunk * SPK_CHUNK_ROWS + step * 4u + g;
    unsigned int any = 0;
    if (r < sp.count) {
      const uint64_t row = (uint64_t)sp.row_lo + r;
      if (spk_row_id(sp, row) != SM_EMPTY) {
        if (lane < (uint32_t)SS_FIELDS) any = smk_load64(sp.acc + row * SS_FIELDS + lane) != 0ull;
        if (sp.hist) {
          const unsigned int* h = sp.hist + row * sp.width;
          for (uint32_t w = lane; w < sp.width; w += SMK_LANES) any |= smk_load32(h + w) != 0u;
        }
      }
    }
    const unsigned long long votes = __ballot(any != 0);
    for (uint32_t q = 0; q < 4; ++q)
      if ((votes >> (q * SMK_LANES)) & 0xFFFFull) mask |= 1ull << (step * 4u + q);
  }
  if (wl == 0) sp.mask[chunk] = mask;
}

// one workgroup. Thread t of a step owns the chunks base + 4 t .. base + 4 t + 3: their popcounts, an inclusive scan across the
// wave by shuffles, the four waves' sums through LDS, the carry of the steps before.
__global__ __launch_bounds__(256) void k_site_pack_scan(SitePack sp) {
  __shared__ uint32_t wave_sum[SPK_CHUNKS_PER_BLOCK];
  const uint32_t chunks = (sp.count + SPK_CHUNK_ROWS - 1) / SPK_CHUNK_ROWS;
  const uint32_t wv = threadIdx.x / 64u, wl = threadIdx.x % 64u;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < chunks; base += SPK_SCAN_TILE) {
    const uint32_t c0 = base + threadIdx.x * SPK_SCAN_PER_THREAD;
    uint32_t n[SPK_SCAN_PER_THREAD], mine = 0;
#pragma unroll
    for (int k = 0; k < SPK_SCAN_PER_THREAD; ++k) {
      n[k] = c0 + k < chunks ? (uint32_t)__popcll(sp.mask[c0 + k]) : 0u;
      mine += n[k];
    }
    uint32_t inc = mine;
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = (uint32_t)__shfl_up((int)inc, d, 64);
      if (wl >= (uint32_t)d) inc += o;
    }
    if (wl == 63u) wave_sum[wv] = inc;
    __syncthreads();
    uint32_t at = carry + inc - mine, tile = 0;
    for (uint32_t i = 0; i < (uint32_t)SPK_CHUNKS_PER_BLOCK; ++i) {
      if (i < wv) at += wave_sum[i];
      tile += wave_sum[i];
    }
#pragma unroll
    for (int k = 0; k < SPK_SCAN_PER_THREAD; ++k)
      if (c0 + k < chunks) {
        sp.offset[c0 + k] = at;
        at += n[k];
      }
    carry += tile;
    __syncthreads();  // (wave_sum is written again by the next step)
  }
  if (threadIdx.x == 0) *sp.total = carry;
}

// the grid of k_site_pack_count; cap: the records the output holds (a live row past it is not written)
__global__ __launch_bounds__(256) void k_site_pack_write(SitePack sp) {
  const uint32_t chunk = blockIdx.x * (uint32_t)SPK_CHUNKS_PER_BLOCK + threadIdx.x / 64u;
  const uint32_t wl = threadIdx.x % 64u, g = wl / SMK_LANES, lane = wl % SMK_LANES;
  if (chunk >= (sp.count + SPK_CHUNK_ROWS - 1) / SPK_CHUNK_ROWS) return;
  const unsigned long long mask = sp.mask[chunk];
  if (!mask) return;
  const uint32_t first = sp.offset[chunk];
  for (uint32_t step = 0; step < SPK_CHUNK_ROWS / 4; ++step) {
    const uint32_t bit = step * 4u + g;
    if (!((mask >> bit) & 1ull)) continue;
    const uint64_t o = (uint64_t)first + (uint32_t)__popcll(mask & ((1ull << bit) - 1ull));
    if (o >= sp.cap) continue;
    const uint64_t row = (uint64_t)sp.row_lo + chunk * SPK_CHUNK_ROWS + bit;
    if (lane == 0) sp.out_site[o] = sp.keys ? sm_load_key(sp.keys, (uint32_t)row) : (uint32_t)row;
    if (lane < (uint32_t)SS_FIELDS) sp.out_cells[o * SS_FIELDS + lane] = smk_load64(sp.acc + row * SS_FIELDS + lane);
    if (sp.hist) {
      const unsigned int* src = sp.hist + row * sp.width;
      unsigned int* dst = sp.out_hist + o * sp.width;
      for (uint32_t w = lane; w < sp.width; w += SMK_LANES) dst[w] = smk_load32(src + w);
    }
  }
}

inline bool site_pack_ready(const SitePack& sp) {
  return sp.acc && sp.mask && sp.offset && sp.total && sp.count != 0 && sp.count <= (1u << 20) && (!sp.hist || sp.width != 0);
}

// the count and the scan of one window, back to back: *sp.total is the window's live rows
inline void launch_site_pack_kernels(const SitePack& sp, hipStream_t s) {
  if (!site_pack_ready(sp)) return;
  const unsigned chunks = (sp.count + SPK_CHUNK_ROWS - 1) / SPK_CHUNK_ROWS;
  hipLaunchKernelGGL(k_site_pack_count, dim3((chunks + SPK_CHUNKS_PER_BLOCK - 1) / SPK_CHUNKS_PER_BLOCK), dim3(256), 0, s, sp);
  hipLaunchKernelGGL(k_site_pack_scan, dim3(1), dim3(256), 0, s, sp);
}

// the write behind them, into records sized from *sp.total
inline void launch_site_pack_write_kernel(const SitePack& sp, hipStream_t s) {
  if (!site_pack_ready(sp) || !sp.cap || !sp.out_site || !sp.out_cells || (sp.hist && !sp.out_hist)) return;
  const unsigned chunks = (sp.count + SPK_CHUNK_ROWS - 1) / SPK_CHUNK_ROWS;
  hipLaunchKernelGGL(k_site_pack_write, dim3((chunks + SPK_CHUNKS_PER_BLOCK - 1) / SPK_CHUNKS_PER_BLOCK), dim3(256), 0, s, sp);
}

// grid ceil(count / 16): lanes [16 g, 16 g + 16) of a block own record blockIdx.x * 16 + g. The body behind the row is
// k_site_scatter_add's, REPEATED here and not shared: that kernel is to keep its source, so a change to what either adds (a new
// field, another carry) has to be made in both, and tests/test_gpu_site_pack.py (the same records through both into the same
// windows) is what tells when they drift.
__global__ __launch_bounds__(256) void k_site_merge(SiteMerge sm) {
  const uint32_t t = blockIdx.x * (uint32_t)SMK_SITES_PER_BLOCK + threadIdx.x / SMK_LANES;
  const uint32_t lane = threadIdx.x % SMK_LANES;
  const bool live = t < sm.count;  // (no early return: the whole group takes part in the shuffles below)
  const unsigned long long* __restrict__ src = sm.cells + (uint64_t)t * SS_FIELDS;
  const unsigned int* __restrict__ cnt = sm.counters + (uint64_t)t * sm.width;
  unsigned int any = 0;
  if (live) {
    if (lane < (uint32_t)SS_FIELDS) any = src[lane] != 0ull;
    if (sm.hist)
      for (uint32_t w = lane; w < sm.width; w += SMK_LANES) any |= cnt[w] != 0u;
  }
  for (int d = SMK_LANES >> 1; d > 0; d >>= 1) any |= (unsigned int)__shfl_xor((int)any, d, SMK_LANES);
  uint32_t row = SM_NO_ROW;
  if (any && lane == 0) {
    const uint64_t id = (uint64_t)sm.site[t] + sm.offset;
    if (id < sm.num_sites) {  // (the host has refused every other id: nothing is ever added outside the table)
      if (sm.keys) {
        row = sm_find_or_insert(sm.keys, sm.capacity, sm.stats, (uint32_t)id);
        if (row == SM_NO_ROW) atomicAdd(sm.stats + SM_SITES_DROPPED, 1ull);
      } else {
        row = (uint32_t)id;
      }
    }
  }
  row = (uint32_t)__shfl((int)row, 0, SMK_LANES);
  if (row != SM_NO_ROW) {
    unsigned long long* cell = sm.acc + (uint64_t)row * SS_FIELDS;
    if (lane < 3) {
      if (src[lane]) atomicAdd(cell + lane, src[lane]);
    } else if (lane == 3) {
      xs_add128(cell + 3, src[3], src[4]);
    } else if (lane == 4) {
      xs_add128(cell + 5, src[5], src[6]);
    }
    if (sm.hist) {
      unsigned int* h = sm.hist + (uint64_t)row * sm.width;
      for (uint32_t w = lane; w < sm.width; w += SMK_LANES) {
        const unsigned int v = cnt[w];
        if (v) atomicAdd(h + w, v);
      }
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && sm.add_totals)
    for (int f = 0; f < SS_TOTALS; ++f)
      if (sm.totals_in[f]) atomicAdd(sm.totals + f, sm.totals_in[f]);
}

inline void launch_site_merge_kernel(const SiteMerge& sm, hipStream_t s) {
  // (no record: the totals alone, by thread 0 of one workgroup -- the staged arrays are then not looked at)
  if (!sm.acc || !sm.totals || (sm.count == 0 ? !sm.add_totals : (!sm.site || !sm.cells)) || sm.num_sites == 0 ||
      (sm.keys && (!sm.capacity || !sm.stats)) || (sm.count && sm.hist && (!sm.counters || sm.width == 0)))
    return;
  const unsigned blocks = sm.count ? (sm.count + SMK_SITES_PER_BLOCK - 1) / SMK_SITES_PER_BLOCK : 1u;
  hipLaunchKernelGGL(k_site_merge, dim3(blocks), dim3(256), 0, s, sm);
}

}  // namespace dynk
