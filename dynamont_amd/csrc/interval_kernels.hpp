// interval_kernels.hpp -- per-border credible intervals (dyn_aligner_set_border_interval): for every lattice column n >= 1 the
// masses exp(LPM(t, n)) over the rows t are the distribution of "base n starts at row t"; its two quantiles (1 - mass) / 2 and
// 1 - (1 - mass) / 2 and its first two moments are the four output columns. Included by nt_kernels.hip and band_reads.hip (the
// phase behind traceback / mpost, where the border-confidence phase runs, while the read's lattice is still in its pages or
// arena) and by tests/device_math/border_interval.hip, which runs both sweeps on a lattice the test writes itself.
//
// Definition (include/dynamont_mi.h). Output row j of an ok read is lattice column n = j + 1, the row of
// its M cell is r = segrow[j]; LPM(t, n) is what the border-confidence accessors (border_kernels.hpp, used here unedited) return:
// -inf outside the reference's band window of row t and in row 0. p(t) = exp(LPM(t, n)), 0 where LPM is -inf, t = 1 .. T-1,
// a = (1 - mass) / 2. All sums fp64, ascending t, one IEEE add per term, no contraction:
//   C(t) running sum of p;  S = C(T-1);  A = sum of d * p, d = t - r (one __dmul_rn);  B = sum of (d * d) * p (d * d first)
//   border_lo    (first t with C(t) >= a) - 1          } absolute thresholds: one pass. A threshold no row reaches: the last
//   border_hi    (first t with C(t) >= 1 - a) - 1      } in-band row of the column, minus 1
//   border_mean  (r - 1) + A / S
//   border_sd    sqrt(max(B / S - (A / S)^2, 0))
// A row outside the column's band interval contributes +-0.0 to every sum and leaves its bits as they are, so the sums over
// the in-band rows alone -- what both sweeps form -- are the sums of the definition.
//
// Lane mapping in the read queue (interval_sweep_wave, one wave per read): the wave walks ABSOLUTE rows t = 1 .. T-1, and every
// lane owns the CPL = 7 band slots the register sweeps gave it (slot = n mod 448 = lane * 7 + j). 2 bw + 1 <= 447, so a slot
// holds at most one in-band column in any row, and start(t) is monotone, so a column's in-band rows are one interval: a lane
// keeps (C, A, B, lo, hi, last row, column, r) per slot in registers, and when the slot's column changes, or the read ends, it
// hands the finished column to the sink and starts afresh. For one j the 64 lanes read 64 neighbouring positions of ONE stored
// row (border_row_pos) in one instruction -- where the border-confidence phase, one lane per column, moves a cache line per
// load. The seven terms of a row, and of IV_ROWS rows at a time, are evaluated side by side (the accessors take no branch around
// their loads).
// Banded-lattice kernel (interval_column_walk): one thread per column walking that column's row interval, the correctness path.
// No atomics, no LDS, no scratch memory (every per-slot array is indexed by unrolled constants); no result depends on anything
// but the read's own lattice: the same bits run to run.
#pragma once

#include "border_kernels.hpp"

namespace dynk {

// the state of one column while its rows go by
struct IntervalColumn {
  double C, A, B;
  uint32_t lo, hi, last;  // lattice rows (>= 1); 0: the threshold is not reached yet / no row seen yet
  __device__ __forceinline__ void clear() {
    C = A = B = 0.0;
    lo = hi = last = 0u;
  }
  // row t of the column (in band), p = its mass; r = the row of the called border
  __device__ __forceinline__ void add(int t, int r, double p, double q_lo, double q_hi) {
    const double d = (double)(t - r);
    C = __dadd_rn(C, p);
    A = __dadd_rn(A, __dmul_rn(d, p));
    B = __dadd_rn(B, __dmul_rn(__dmul_rn(d, d), p));
    lo = (lo == 0u && C >= q_lo) ? (uint32_t)t : lo;
    hi = (hi == 0u && C >= q_hi) ? (uint32_t)t : hi;
    last = (uint32_t)t;
  }
  // the two quantiles as signal positions (row - 1); a column without an in-band row (no ok read has one) gives 0
  __device__ __forceinline__ uint32_t lo_pos() const { const uint32_t t = lo ? lo : last; return t ? t - 1u : 0u; }
  __device__ __forceinline__ uint32_t hi_pos() const { const uint32_t t = hi ? hi : last; return t ? t - 1u : 0u; }
};

// the sink of the product's kernels: the four values of column n at output row `at`
__device__ __forceinline__ void interval_store(const IntervalOut& o, size_t at, const IntervalColumn& c, int r) {
  const bool any = c.C > 0.0;  // (the called border itself lies in the column: S > 0 for every column of an ok read)
  const double m = any ? __ddiv_rn(c.A, c.C) : 0.0;
  const double v = any ? __dsub_rn(__ddiv_rn(c.B, c.C), __dmul_rn(m, m)) : 0.0;
  o.mean[at] = __dadd_rn((double)(r - 1), m);
  o.mean[o.capacity + at] = __dsqrt_rn(v > 0.0 ? v : 0.0);
  uint32_t* q = reinterpret_cast<uint32_t*>(o.mean + 2 * o.capacity);
  q[at] = c.lo_pos();
  q[o.capacity + at] = c.hi_pos();
}

constexpr int IV_ROWS = 2;  // rows whose loads are in flight together

// the read-queue sweep: called by ONE WHOLE WAVE (lane = 0 .. 63). rows[n - 1] = r of column n (the read's part of segrow);
// sink(n, column, r) is called once per column n = 1 .. N-1 that has an in-band row, by the lane that owns its slot.
template <class CELL, class SINK>
__device__ __forceinline__ void interval_sweep_wave(const CELL& cell, const BorderBand& band, const uint32_t* rows, double tail,
                                                    int lane, const SINK& sink) {
  const int T = band.T, N = band.N;
  const double q_lo = tail, q_hi = __dsub_rn(1.0, tail);
  IntervalColumn col[CPL];
  int cur[CPL], r[CPL];
#pragma unroll
  for (int j = 0; j < CPL; ++j) {
    col[j].clear();
    cur[j] = 0;  // column 0 holds nothing: "no column"
    r[j] = 0;
  }
#pragma unroll 1
  for (int t = 1; t < T; t += IV_ROWS) {
    // IV_ROWS rows at a time: their terms are evaluated side by side (the loads of all of them in flight together), then added
    // in row order. A row past the last one holds no column: it ends every column that is still open, as the read's end does.
    int nn[IV_ROWS][CPL];
    double p[IV_ROWS][CPL];
#pragma unroll
    for (int u = 0; u < IV_ROWS; ++u) {
      const bool live = t + u < T;
      const int tu = live ? t + u : T - 1;
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
        p[u][j] = border_term(cell, tu, nn[u][j] ? n : n_lo);
      }
    }
#pragma unroll
    for (int u = 0; u < IV_ROWS; ++u) {
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        if (nn[u][j] != cur[j]) {
          if (cur[j]) sink(cur[j], col[j], r[j]);
          cur[j] = nn[u][j];
          col[j].clear();
          if (nn[u][j]) r[j] = (int)rows[nn[u][j] - 1];
        }
        if (nn[u][j]) col[j].add(t + u, r[j], p[u][j], q_lo, q_hi);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < CPL; ++j)
    if (cur[j]) sink(cur[j], col[j], r[j]);
}

// one thread, one column: the rows the column can be in band at follow from centre(t) = floor(t * ratio) in [n - bw, n + bw]; the
// estimate is taken a row wide on either side and every row is asked (BorderBand::holds), so only its being wide enough matters
template <class CELL>
__device__ __forceinline__ void interval_column_walk(const CELL& cell, const BorderBand& band, int n, int r, double tail, IntervalColumn& col) {
  const double q_lo = tail, q_hi = __dsub_rn(1.0, tail);
  const double first = (double)(n - band.bw) / band.ratio, beyond = (double)(n + band.bw + 1) / band.ratio;
  const int t0 = first > 3.0 ? (int)first - 2 : 1;
  const int t1 = beyond + 2.0 < (double)(band.T - 1) ? (int)beyond + 2 : band.T - 1;
  col.clear();
#pragma unroll 1
  for (int t = t0; t <= t1; ++t) {
    if (!band.holds(t, n)) continue;
    col.add(t, r, border_term(cell, t, n), q_lo, q_hi);
  }
}

// the phase of the read queue: every column of the read, by one whole wave
template <class CELL>
__device__ __forceinline__ void border_interval_read_wave(const CELL& cell, const BorderBand& band, const ReadDesc& rd,
                                                          const uint32_t* __restrict__ segrow, const IntervalOut& out, int lane) {
  if (band.N < 2) return;
  const size_t at0 = rd.seg_off;
  interval_sweep_wave(cell, band, segrow + at0, out.tail, lane,
                      [&](int n, const IntervalColumn& c, int r) { interval_store(out, at0 + (size_t)(n - 1), c, r); });
}

// the phase of the banded-lattice kernel: one column per thread of the `n_threads` that call this (tid = 0 .. n_threads-1)
template <class CELL>
__device__ __forceinline__ void border_interval_read_columns(const CELL& cell, const BorderBand& band, const ReadDesc& rd,
                                                             const uint32_t* __restrict__ segrow, const IntervalOut& out, int tid,
                                                             int n_threads) {
  for (int n = 1 + tid; n < band.N; n += n_threads) {
    const int r = (int)segrow[rd.seg_off + n - 1];
    IntervalColumn c;
    interval_column_walk(cell, band, n, r, out.tail, c);
    interval_store(out, rd.seg_off + (size_t)(n - 1), c, r);
  }
}

}  // namespace dynk
