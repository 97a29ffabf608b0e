// soft_level_kernels.hpp -- posterior-weighted per-base levels and expected dwell (dyn_aligner_set_soft_levels): for every lattice
// column n >= 1 the posterior that sample t-1 belongs to base n, g(t) = exp(LPM(t, n)) + exp(LPE(t, n)), summed over the rows as
// a weight (the expected dwell) and the first two moments of the signal under it -- the per-base terms of train()'s per-k-mer
// sums. Included by nt_kernels.hip and band_reads.hip (the phase behind traceback / mpost, where the other lattice phases run,
// while the read's lattice is still in its pages or arena) and by tests/device_math/soft_levels.hip, which runs both sweeps on a
// lattice the test writes itself.
//
// Definition (include/dynamont_mi.h). Output row j of an ok read is lattice column n = j + 1. LPM(t, n)
// is what the border-confidence accessors (border_kernels.hpp) return, LPE(t, n) what the sampling accessors (sample_kernels.hpp)
// return, both used here unedited: -inf outside the reference's band window of row t and in row 0. x = the signal the lattice
// was computed on, x[t - 1] belongs to row t. All sums fp64, ascending t = 1 .. T-1, one IEEE operation per step, no contraction:
//   pM = exp(LPM), pE = exp(LPE) (0 where the log is -inf);  g = pM + pE (formed first)
//   soft_weight += g;   soft_sum += g * x;   soft_sumsq += (g * x) * x     (the reference's grouping: posterior * obs * obs)
// A row outside the column's band interval would add +0.0 to every sum and leave its bits as they are, so the sums over the
// in-band rows alone -- what both sweeps form -- are the sums of the definition.
//
// Lane mapping in the read queue (soft_sweep_wave, one wave per read): interval_sweep_wave's. The wave walks ABSOLUTE rows
// t = 1 .. T-1, and every lane owns the CPL = 7 band slots the register sweeps gave it (slot = n mod 448 = lane * 7 + j).
// 2 bw + 1 <= 447, so a slot holds at most one in-band column in any row, and start(t) is monotone, so a column's in-band rows
// are one interval: a lane keeps (weight, sum, sumsq, column) per slot in registers, and when the slot's column changes, or the
// read ends, it hands the finished column to the sink and starts afresh. For one j the 64 lanes read 64 neighbouring positions
// of ONE stored row in one instruction; x[t - 1] is uniform over the wave. The seven terms of a row, and of SL_ROWS rows at a
// time, are evaluated side by side (the accessors take no branch around their loads), then added in row order.
// Banded-lattice kernel (soft_column_walk): one thread per column walking that column's row interval, the correctness path.
// No atomics, no LDS, no scratch memory (every per-slot array is indexed by unrolled constants); no result depends on anything
// but the read's own lattice and signal: the same bits run to run.
#pragma once

#include "border_kernels.hpp"
#include "sample_kernels.hpp"

namespace dynk {

// the state of one column while its rows go by
struct SoftColumn {
  double w, s1, s2;
  __device__ __forceinline__ void clear() { w = s1 = s2 = 0.0; }
  // row t of the column (in band): g = its posterior, x = the row's sample
  __device__ __forceinline__ void add(double g, double x) {
    const double gx = __dmul_rn(g, x);
    w = __dadd_rn(w, g);
    s1 = __dadd_rn(s1, gx);
    s2 = __dadd_rn(s2, __dmul_rn(gx, x));
  }
};

// one term of the sums: the posterior of cell (t, n), the M and the E share added once
template <class LPM, class LPE>
__device__ __forceinline__ double soft_term(const LPM& cell_lpm, const LPE& cell_lpe, int t, int n) {
  return __dadd_rn(border_term(cell_lpm, t, n), border_term(cell_lpe, t, n));
}

// the sink of the product's kernels: the three sums of column n at output row `at`
__device__ __forceinline__ void soft_store(const SoftOut& o, size_t at, const SoftColumn& c) {
  o.weight[at] = c.w;
  o.weight[o.capacity + at] = c.s1;
  o.weight[2 * o.capacity + at] = c.s2;
}

constexpr int SL_ROWS = 2;  // rows whose loads are in flight together

// the read-queue sweep: called by ONE WHOLE WAVE (lane = 0 .. 63). sg = the read's samples (sg[t - 1] belongs to row t);
// sink(n, column) is called once per column n = 1 .. N-1 that has an in-band row, by the lane that owns its slot.
template <class LPM, class LPE, class SINK>
__device__ __forceinline__ void soft_sweep_wave(const LPM& cell_lpm, const LPE& cell_lpe, const BorderBand& band,
                                                const double* __restrict__ sg, int lane, const SINK& sink) {
  const int T = band.T, N = band.N;
  SoftColumn col[CPL];
  int cur[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    col[j].clear();
    cur[j] = 0;  // column 0 holds nothing: "no column"
  }
#pragma unroll 1
  for (int t = 1; t < T; t += SL_ROWS) {
    // SL_ROWS rows at a time: their terms are evaluated side by side (the loads of all of them in flight together), then added
    // in row order. A row past the last one holds no column: it ends every column that is still open, as the read's end does.
    int nn[SL_ROWS][CPL];
    double g[SL_ROWS][CPL], x[SL_ROWS];
#pragma unroll
    for (int u = 0; u < SL_ROWS; ++u) {
      const bool live = t + u < T;
      const int tu = live ? t + u : T - 1;
      x[u] = sg[tu - 1];
      // the band window of the row: columns [n_lo, n_hi), never empty (1 <= n_lo < N)
      const int s0 = band.start(tu);
      const int n_lo = s0 > 1 ? s0 : 1;
      const int n_hi = s0 + 2 * band.bw + 1 < N ? s0 + 2 * band.bw + 1 : N;
      const int base = n_lo - n_lo % P;
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        // the one column of [n_lo, n_lo + 448) that lives in this slot; outside the window the term is evaluated at n_lo, whose
        // every address is the read's own, and dropped
        const int k = base + lane * CPL + j;
        const int n = k < n_lo ? k + P : k;
        nn[u][j] = (live && n < n_hi) ? n : 0;
        g[u][j] = soft_term(cell_lpm, cell_lpe, tu, nn[u][j] ? n : n_lo);
      }
    }
#pragma unroll
    for (int u = 0; u < SL_ROWS; ++u) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        if (nn[u][j] != cur[j]) {
          if (cur[j]) sink(cur[j], col[j]);
          cur[j] = nn[u][j];
          col[j].clear();
        }
        if (nn[u][j]) col[j].add(g[u][j], x[u]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j)
    if (cur[j]) sink(cur[j], col[j]);
}

// one thread, one column: the rows the column can be in band at follow from centre(t) = floor(t * ratio) in [n - bw, n + bw]; the
// estimate is taken a row wide on either side and every row is asked (BorderBand::holds), so only its being wide enough matters
template <class LPM, class LPE>
__device__ __forceinline__ void soft_column_walk(const LPM& cell_lpm, const LPE& cell_lpe, const BorderBand& band,
                                                 const double* __restrict__ sg, int n, SoftColumn& col) {
  const double first = (double)(n - band.bw) / band.ratio, beyond = (double)(n + band.bw + 1) / band.ratio;
  const int t0 = first > 3.0 ? (int)first - 2 : 1;
  const int t1 = beyond + 2.0 < (double)(band.T - 1) ? (int)beyond + 2 : band.T - 1;
  col.clear();
#pragma unroll 1
  for (int t = t0; t <= t1; ++t) {
    if (!band.holds(t, n)) continue;
    col.add(soft_term(cell_lpm, cell_lpe, t, n), sg[t - 1]);
  }
}

// the phase of the read queue: every column of the read, by one whole wave
template <class LPM, class LPE>
__device__ __forceinline__ void soft_levels_read_wave(const LPM& cell_lpm, const LPE& cell_lpe, const BorderBand& band,
                                                      const ReadDesc& rd, const double* __restrict__ sg, const SoftOut& out, int lane) {
  if (band.N < 2) return;
  const size_t at0 = rd.seg_off;
  soft_sweep_wave(cell_lpm, cell_lpe, band, sg, lane, [&](int n, const SoftColumn& c) { soft_store(out, at0 + (size_t)(n - 1), c); });
}

// the phase of the banded-lattice kernel: one column per thread of the `n_threads` that call this (tid = 0 .. n_threads-1)
template <class LPM, class LPE>
__device__ __forceinline__ void soft_levels_read_columns(const LPM& cell_lpm, const LPE& cell_lpe, const BorderBand& band,
                                                         const ReadDesc& rd, const double* __restrict__ sg, const SoftOut& out, int tid,
                                                         int n_threads) {
  for (int n = 1 + tid; n < band.N; n += n_threads) {
    SoftColumn c;
    soft_column_walk(cell_lpm, cell_lpe, band, sg, n, c);
    soft_store(out, rd.seg_off + (size_t)(n - 1), c);
  }
}

}  // namespace dynk
