// site_summary_kernels.hpp -- the per-site level summary of a run (dyn_aligner_set_site_summary): for every caller-supplied
// site id (a reference position, usually) the coverage, the dwell and the sums of the reads' EVENT MEANS and of their squares,
// as EXACT INTEGERS. Included by site_summary.hip (launch_site_summary) and by tests/device_math/site_summary.hip, which
// feeds the launch path arrays built on the host and compares every integer with a Python-int restatement
// (tests/test_gpu_site_summary.py). The kernels are ordinary (non-inline) definitions: one translation unit per binary
// includes this file.
//
// Definition. Output row j of an ok read covers lattice rows [segrow[j], segrow[j+1]) (the last
// one up to T), i.e. samples row - 1 of the signal the read queue aligned: L samples. Its site is sites[par_off + j] (the
// host put the id of base j + kmer_size / 2 there: the row's sequence_pos).
//   S1       the chunked sum of event_stats.hip (exact_sum_kernels.hpp)
//   m        __ddiv_rn(S1, (double)L): level_mean of dyn_event_out, bit for bit
//   m1, m2   rint(m * 2^40), rint(__dmul_rn(m, m) * 2^40) as exact integers (ties to even; the scaling is exact)
//   no site  id == DYN_SITE_NONE: counted in rows_without_site, not added
//   skipped  id >= num_sites, a non-finite m or m * m >= 2^64 (|m| < 2^32 bounds m1 with it): counted in rows_skipped
// Per site seven u64: n_rows, n_samples = sum L, dwell_sq = sum L * L (mod 2^64), M1 = sum m1 and M2 = sum m2 as 128-bit two's
// complement (low limb, high limb). Integer addition commutes: the atomics below may land in any order and the table is the
// same bits whatever the launch path or the merging of tickets. No float atomics, no sort.
// Two kernels, split like k_ksum_short / k_ksum_long at SS_SHORT_MAX samples, the same summation order:
//   k_ssum_short  one thread per OUTPUT row: block (read, chunk of 256 rows)
//   k_ssum_long   one 256-thread block per read that has a longer row: lanes sum chunks in parallel, lane 0 adds the chunk
//                 sums in order (the chunk loop wraps beyond 256 chunks, rows above 16 384 samples)
// Footprint: 256 threads, 2 KB of static LDS (k_ssum_long), no scratch -- they run beside a resident workgroup.
//
// The per-site histograms (dyn_aligner_set_site_histogram, ss.hist != nullptr): every row the table adds also counts into two
// uint32 counters of its site's H = bins + 2 + 16 contiguous ones, [under, level bin 1 .. bins, over, dwell bin 0 .. 15]:
//   level  u = __dmul_rn(__dsub_rn(m, lo), inv_w); u < 0: 0; u >= bins: bins + 1; otherwise 1 + (int)u
//   dwell  min(31 - clz(L), 15)
// with 32-bit device-scope atomics: exact while a site has fewer than 2^32 rows. k_site_quantiles reduces a window of the level
// histograms to ranks and bins on the device (site_quantile_kernels.hpp).
//
// The sparse mode (dyn_aligner_set_site_summary_sparse, ss.map_keys != nullptr): acc and hist have ss.capacity rows, and a row
// that passed every check above looks its id up in the map (site_map.hpp), inserting it when it is new; the bucket is the row.
// A row whose id finds no bucket in its probe window is dropped: counted in map_stats[rows_dropped] and in rows_skipped.
#pragma once

#include "exact_sum_kernels.hpp"
#include "nt_kernels.hpp"
#include "site_map.hpp"

namespace dynk {

constexpr int SS_SHORT_MAX = 256;
constexpr uint32_t SS_SITE_NONE = 0xFFFFFFFFu;

// one row into its site's cell (id < num_sites); returns false when the definition skips it
__device__ __forceinline__ bool ss_accumulate(const SiteSummary& ss, uint32_t id, int L, double s1) {
  const double m = __ddiv_rn(s1, (double)L);
  const double mm = __dmul_rn(m, m);
  if (!(mm < XS_TWO64)) return false;  // NaN and +-inf fail the comparison too
  if (ss.map_keys) {  // sparse: the row of the id, taken now when the id is new; a row left out above never inserts a key
    const uint32_t row = sm_find_or_insert(ss.map_keys, ss.capacity, ss.map_stats, id);
    if (row == SM_NO_ROW) {  // dropped: counted here and, by the caller, in rows_skipped
      atomicAdd(ss.map_stats + SM_ROWS_DROPPED, 1ull);
      return false;
    }
    id = row;
  }
  unsigned long long* cell = ss.acc + (uint64_t)id * SS_FIELDS;
  atomicAdd(cell, 1ull);
  atomicAdd(cell + 1, (unsigned long long)L);
  atomicAdd(cell + 2, (unsigned long long)L * (unsigned long long)L);
  unsigned long long lo, hi;
  xs_to_i128(rint(__dmul_rn(m, XS_SCALE)), lo, hi);
  xs_add128(cell + 3, lo, hi);
  xs_to_i128(rint(__dmul_rn(mm, XS_SCALE)), lo, hi);
  xs_add128(cell + 5, lo, hi);
  if (ss.hist) {
    unsigned int* h = ss.hist + (uint64_t)id * (ss.bins + 2u + (uint32_t)SH_DWELL_BINS);
    const double u = __dmul_rn(__dsub_rn(m, ss.hist_lo), ss.inv_w);  // m is finite here, inv_w finite and > 0: u is no NaN
    const uint32_t lb = u < 0.0 ? 0u : (u >= (double)ss.bins ? ss.bins + 1u : 1u + (uint32_t)(int)u);
    atomicAdd(h + lb, 1u);
    atomicAdd(h + ss.bins + 2u + (uint32_t)min(31 - __clz(L), SH_DWELL_BINS - 1), 1u);
  }
  return true;
}

__device__ __forceinline__ bool ss_read_wanted(const SiteSummary& ss, const ReadDesc& rd, const ReadState* __restrict__ st) {
  return rd.read >= ss.read_lo && rd.read < ss.read_hi && st[rd.read].status == 0;
}

// grid (n_reads, ceil((max_N - 1) / 256)): thread j of block (r, c) owns output row c * 256 + j of read descs[r]
__global__ __launch_bounds__(256) void k_ssum_short(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                    const uint32_t* __restrict__ segrow_all, SiteSummary ss) {
  const ReadDesc rd = descs[blockIdx.x];
  const int n_seg = (int)rd.N - 1;
  if ((int)(blockIdx.y * 256u) >= n_seg) return;  // (an ok read has at least one row, N >= 2: block y = 0 always gets past this)
  if (!ss_read_wanted(ss, rd, st)) return;
  const int T = (int)rd.T;
  const int j = (int)(blockIdx.y * 256u + threadIdx.x);
  unsigned long long n_kept = 0, n_samp = 0, n_none = 0, n_skip = 0;
  if (j < n_seg) {
    const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
    const int a = (int)segrow[j];
    const int b = (j + 1 < n_seg) ? (int)segrow[j + 1] : T;
    const int L = b - a;
    if (L >= 1 && L <= SS_SHORT_MAX && a >= 1 && b <= T) {
      const uint32_t id = ss.sites[rd.par_off + j];
      if (id == SS_SITE_NONE) {
        n_none = 1;
      } else if (id >= ss.num_sites) {
        n_skip = 1;
      } else if (ss_accumulate(ss, id, L, xs_chunked_sum(ss.sig + rd.sig_off + (a - 1), L))) {  // sample row - 1
        n_kept = 1;
        n_samp = (unsigned long long)L;
      } else {
        n_skip = 1;
      }
    }
  }
  n_kept = xs_wave_sum(n_kept);
  n_samp = xs_wave_sum(n_samp);
  n_none = xs_wave_sum(n_none);
  n_skip = xs_wave_sum(n_skip);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (n_kept) atomicAdd(ss.totals + 1, n_kept);
    if (n_samp) atomicAdd(ss.totals + 2, n_samp);
    if (n_none) atomicAdd(ss.totals + 3, n_none);
    if (n_skip) atomicAdd(ss.totals + 4, n_skip);
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(ss.totals, 1ull);  // reads_ok
}

__global__ __launch_bounds__(256) void k_ssum_long(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                   const uint32_t* __restrict__ segrow_all, SiteSummary ss) {
  __shared__ double s_p1[256];
  const ReadDesc rd = descs[blockIdx.x];
  if (!ss_read_wanted(ss, rd, st)) return;
  const int T = (int)rd.T, n_seg = (int)rd.N - 1;
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  int any = 0;
  for (int i = tid; i < n_seg; i += 256) {
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    any |= (b - a > SS_SHORT_MAX);
  }
  if (!__syncthreads_or(any)) return;
  for (int i = 0; i < n_seg; ++i) {  // block-uniform walk over the rows of this read
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    const int L = b - a;
    if (L <= SS_SHORT_MAX || a < 1 || b > T) continue;
    const uint32_t id = ss.sites[rd.par_off + i];  // block-uniform: a row without a usable site is counted, not summed
    if (id >= ss.num_sites) {
      if (tid == 0) atomicAdd(ss.totals + (id == SS_SITE_NONE ? 3 : 4), 1ull);
      continue;
    }
    const double* __restrict__ xs = ss.sig + rd.sig_off + (a - 1);
    const int n_chunks = (L + XS_CHUNK - 1) / XS_CHUNK;
    double acc1 = 0.0;  // lane 0's running total
    for (int c0 = 0; c0 < n_chunks; c0 += 256) {
      const int c = c0 + tid;
      if (c < n_chunks) s_p1[tid] = xs_chunked_sum(xs + c * XS_CHUNK, min(XS_CHUNK, L - c * XS_CHUNK));
      __syncthreads();
      if (tid == 0)
        for (int k = 0; k < min(256, n_chunks - c0); ++k) acc1 = (c0 + k == 0) ? s_p1[k] : __dadd_rn(acc1, s_p1[k]);
      __syncthreads();
    }
    if (tid == 0) {
      if (ss_accumulate(ss, id, L, acc1)) {
        atomicAdd(ss.totals + 1, 1ull);
        atomicAdd(ss.totals + 2, (unsigned long long)L);
      } else {
        atomicAdd(ss.totals + 4, 1ull);
      }
    }
  }
}

// the two launches of launch_site_summary (site_summary.hip); descs in processing order, max_N the largest ReadDesc::N
inline void launch_site_summary_kernels(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st,
                                        const uint32_t* segrow, const SiteSummary& ss, hipStream_t s) {
  if (!ss.acc || !ss.sites || n_reads <= 0 || max_N < 2 || ss.num_sites == 0 || ss.read_lo >= ss.read_hi) return;
  const unsigned chunks = (max_N - 1 + 255) / 256;
  hipLaunchKernelGGL(k_ssum_short, dim3((unsigned)n_reads, chunks), dim3(256), 0, s, descs, st, segrow, ss);
  hipLaunchKernelGGL(k_ssum_long, dim3((unsigned)n_reads), dim3(256), 0, s, descs, st, segrow, ss);
}

}  // namespace dynk
