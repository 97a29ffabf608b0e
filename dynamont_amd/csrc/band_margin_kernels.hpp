// band_margin_kernels.hpp -- band-margin diagnostics (dyn_aligner_set_band_margin): how close the called path of a read came to
// a REAL edge of its band, per read as three uint32. Included by band_margin.hip (launch_band_margin) and by
// tests/device_math/band_margin.hip, which feeds the launch path arrays built on the host and compares every integer with a
// Python-int restatement (tests/test_gpu_band_margin.py). The kernels are ordinary (non-inline) definitions: one translation
// unit per binary includes this file.
//
// Definition. Output row j of an ok read is lattice column n = j + 1 and covers lattice rows
// [a_j, b_j) = [segrow[j], segrow[j+1]) (the last one up to T); mid(t) = dynband::band_mid(t, ratio), bw = ReadDesc::bw.
//   lower edge   real at row t iff mid(t) - bw >= 2 (a column of 1 .. N-1 below the band is excluded); slack n - (mid(t) - bw)
//   upper edge   real at row t iff mid(t) + bw + 1 < N;                                                slack (mid(t) + bw) - n
//   an edge that is not real is the lattice's own border and contributes nothing
//   low, high    the minimum slack over the path rows [a_0, T) where that edge is real; BM_NONE where it never is
//   edge_rows    the path rows with a real slack of 0 (a row where both are 0 counts once)
// A read that failed keeps BM_NONE, BM_NONE, 0 (k_bmargin_init).
// mid is a non-decreasing staircase, n is constant within a segment and both predicates are monotone in t: a segment's lower
// minimum sits on its LAST row and its upper minimum on its FIRST row, and its rows of slack 0 are the rows where mid equals
// n + bw (lower) or n - bw (upper) -- one run of the staircase each, found with dynband::first_row_reaching. One thread per
// OUTPUT row therefore does a constant amount of work whatever the segment's length (tests/test_band_margin_host.py proves the
// shortcut against the all-rows definition).
// The wave reduces by shuffles and issues at most one atomicMin / atomicMin / atomicAdd on uint32: integer min and add
// commute, so the result is the same bits on every launch path. The only floating-point operation that decides anything is
// band_mid's one product (the seed of first_row_reaching is confirmed with band_mid itself).
// Footprint: 256 threads, no LDS, no scratch -- the kernels run beside a resident workgroup.
#pragma once

#include "band_runs.hpp"
#include "nt_kernels.hpp"

namespace dynk {

constexpr uint32_t BM_NONE = 0xffffffffu;  // DYN_BAND_MARGIN_NONE

__device__ __forceinline__ bool bm_read_in_range(const BandMargin& bm, uint32_t read) {
  return read >= bm.read_lo && read < bm.read_hi;
}

// rows t of [a, b) with band_mid(t) == m (a < b; the staircase is monotone, so they are one run)
__device__ __forceinline__ uint32_t bm_rows_at(int m, int a, int b, double ratio, double inv_ratio) {
  if (m < 0 || dynband::band_mid(b - 1, ratio) < m || dynband::band_mid(a, ratio) > m) return 0u;
  const int lo = dynband::first_row_reaching(m, ratio, inv_ratio, a, b - 1);
  const int hi = dynband::band_mid(b - 1, ratio) > m ? dynband::first_row_reaching(m + 1, ratio, inv_ratio, lo, b - 1) : b;
  return (uint32_t)(hi - lo);
}

// grid ceil((read_hi - read_lo) / 256): the reads of the range start from "no real edge met, no row on one"
__global__ __launch_bounds__(256) void k_bmargin_init(BandMargin bm) {
  const uint64_t i = (uint64_t)bm.read_lo + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= bm.read_hi) return;
  bm.low[i] = BM_NONE;
  bm.high[i] = BM_NONE;
  bm.edge_rows[i] = 0u;
}

// grid (n_reads, ceil((max_N - 1) / 256)): thread j of block (r, c) owns output row c * 256 + j of read descs[r]
__global__ __launch_bounds__(256) void k_bmargin(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                 const uint32_t* __restrict__ segrow_all, BandMargin bm) {
  const ReadDesc rd = descs[blockIdx.x];
  const int n_seg = (int)rd.N - 1;
  if ((int)(blockIdx.y * 256u) >= n_seg) return;
  if (!bm_read_in_range(bm, rd.read) || st[rd.read].status != 0) return;
  const int T = (int)rd.T, N = (int)rd.N, bw = (int)rd.bw;
  const int j = (int)(blockIdx.y * 256u + threadIdx.x);
  uint32_t low = BM_NONE, high = BM_NONE, edge = 0u;
  if (j < n_seg) {
    const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
    const int a = (int)segrow[j];
    const int b = (j + 1 < n_seg) ? (int)segrow[j + 1] : T;
    const int n = j + 1;
    if (a >= 0 && a < b && b <= T) {
      const double ratio = rd.ratio;
      const int m_last = dynband::band_mid(b - 1, ratio), m_first = dynband::band_mid(a, ratio);
      if (m_last - bw >= 2) low = (uint32_t)(n - (m_last - bw));
      if (m_first + bw + 1 < N) high = (uint32_t)((m_first + bw) - n);
      // slack 0 below: mid == n + bw, real iff n >= 2; above: mid == n - bw, real iff n + 1 < N
      const double inv_ratio = (double)T / (double)N;  // (seeds the search only)
      const bool lo_can = n >= 2, hi_can = n + 1 < N;
      if (lo_can) edge += bm_rows_at(n + bw, a, b, ratio, inv_ratio);
      if (hi_can && !(bw == 0 && lo_can)) edge += bm_rows_at(n - bw, a, b, ratio, inv_ratio);  // bw == 0: the same rows, once
    }
  }
  for (int d = warpSize >> 1; d > 0; d >>= 1) {
    low = min(low, (uint32_t)__shfl_down(low, d));
    high = min(high, (uint32_t)__shfl_down(high, d));
    edge += (uint32_t)__shfl_down(edge, d);
  }
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (low != BM_NONE) atomicMin(bm.low + rd.read, low);
    if (high != BM_NONE) atomicMin(bm.high + rd.read, high);
    if (edge) atomicAdd(bm.edge_rows + rd.read, edge);
  }
}

// the two launches of launch_band_margin (band_margin.hip); descs in processing order, max_N the largest ReadDesc::N
inline void launch_band_margin_kernels(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st,
                                       const uint32_t* segrow, const BandMargin& bm, hipStream_t s) {
  if (!bm.low || bm.read_lo >= bm.read_hi) return;
  hipLaunchKernelGGL(k_bmargin_init, dim3((bm.read_hi - bm.read_lo + 255u) / 256u), dim3(256), 0, s, bm);
  if (n_reads <= 0 || max_N < 2) return;
  const unsigned chunks = (max_N - 1 + 255) / 256;
  hipLaunchKernelGGL(k_bmargin, dim3((unsigned)n_reads, chunks), dim3(256), 0, s, descs, st, segrow, bm);
}

}  // namespace dynk
