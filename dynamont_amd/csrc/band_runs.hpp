// band_runs.hpp -- where the band window of the sweeps moves, computed instead of tested row by row.
//
// The band of lattice row t is centred on band_mid(t) = size_t(t * RATIO) (NT_aligner_api.cpp:100): one IEEE fp64
// multiply, then truncation. RATIO = N / T <= 1, so the centre is a non-decreasing staircase that climbs at most one
// column per row, and the sweeps' row loops run over the RUNS of rows between two steps with no window test inside.
// Shared by the HIP kernels and by a host-side test (tests/test_band_runs_host.py compiles it with g++ and compares
// it against the row-by-row scan for every input it draws).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DYN_BR_HD __host__ __device__ __forceinline__
#else
#define DYN_BR_HD inline
#endif

namespace dynband {

// the reference's band centre: the product is rounded once (no contraction: there is nothing to contract with)
DYN_BR_HD int band_mid(int t, double ratio) {
#if defined(__HIP_DEVICE_COMPILE__)
  return (int)__dmul_rn((double)t, ratio);
#else
  return (int)((double)t * ratio);
#endif
}

// The first row q in [lo_row, hi_row] with band_mid(q) >= m; the caller knows that band_mid(hi_row) >= m.
// inv_ratio ~ 1 / ratio (any accuracy: it only seeds the search). Predicted with one multiply, then CONFIRMED with
// band_mid itself: the staircase is monotone (rounding and truncation are), so q is pinned by
// band_mid(q) >= m > band_mid(q - 1), and the two loops below walk the prediction onto it whatever its error (0 or 1
// steps for the ratios of real reads).
DYN_BR_HD int first_row_reaching(int m, double ratio, double inv_ratio, int lo_row, int hi_row) {
  const double guess = (double)m * inv_ratio;
  int q = guess < (double)hi_row ? (int)guess : hi_row;  // (a NaN or huge guess lands on hi_row)
  if (q < lo_row) q = lo_row;
  while (band_mid(q, ratio) < m) ++q;  // ends at q <= hi_row
  while (q > lo_row && band_mid(q - 1, ratio) >= m) --q;
  return q;
}

// Forward sweep. The first row r in [t, limit) with band_mid(r + 1) != band_mid(r) -- the row behind which the window
// moves up -- or `limit` when the centre stands still up to there.
DYN_BR_HD int next_move_row(int t, double ratio, double inv_ratio, int limit) {
  if (t >= limit) return limit;
  const int m = band_mid(t, ratio);
  if (band_mid(limit, ratio) == m) return limit;
  return first_row_reaching(m + 1, ratio, inv_ratio, t + 1, limit) - 1;
}

// Backward sweep (rows are consumed top-down). The lowest row q in [floor_row, t] with band_mid(q) == band_mid(t): the
// window moves down in front of row q - 1.
DYN_BR_HD int run_first_row(int t, double ratio, double inv_ratio, int floor_row) {
  if (t <= floor_row) return t;
  return first_row_reaching(band_mid(t, ratio), ratio, inv_ratio, floor_row, t);
}

// ---- runs of row ADDRESSES ---------------------------------------------------------------------------------------------
// A lattice row lives in a page of 2^log_r rows (nt_kernels.hpp), so the address of row t + 1 is the address of row t plus
// a constant for as long as the two share a page. The sweeps carry their row addresses as running values inside a run and
// recompute them from the page table where a run starts, so a run must also end where a cursor would cross a page.

// the first row of the page behind the one that holds row r
DYN_BR_HD int next_page_row(int r, int log_r) { return ((r >> log_r) + 1) << log_r; }

// Forward sweep, two cursors: the row t it writes and the row min(t + ahead, T) it fetches (ahead = 1 + the ring's depth;
// rows past T repeat row T). One past the last row r >= t of [t, limit) such that rows t .. r share a page, rows
// t + ahead .. r + ahead share a page or are all clamped, and t + ahead .. r + ahead lie on one side of the clamp
// (all < T: the fetch address advances by a row per row; all >= T: it stands still).
DYN_BR_HD int fwd_address_run_end(int t, int limit, int log_r, int ahead, int T) {
  if (t >= limit) return limit;
  int end = next_page_row(t, log_r);
  const int d = t + ahead;
  if (d < T) {
    const int page_end = next_page_row(d, log_r) - ahead;  // > t
    const int clamp = T - ahead;                           // > t: the first row whose fetch is row T
    if (page_end < end) end = page_end;
    if (clamp < end) end = clamp;
  }
  return end < limit ? end : limit;
}

// the fetch address of the forward sweep advances inside a run that starts at row t (else every row of it fetches row T)
DYN_BR_HD bool fwd_fetch_advances(int t, int ahead, int T) { return t + ahead < T; }

// Forward sweep: the end of the run that starts at row t -- where the band window moves (next_move_row looks at the rows
// t + 1 .. : the window of row r + 1 differs from that of row r) or an address run ends, whichever comes first.
DYN_BR_HD int fwd_run_end(int t, double ratio, double inv_ratio, int limit, int log_r, int ahead, int T) {
  const int move = next_move_row(t + 1, ratio, inv_ratio, limit);
  const int addr = fwd_address_run_end(t, limit, log_r, ahead, T);
  return move < addr ? move : addr;
}

// Backward sweep (top-down, one cursor: the row t it writes). The lowest row q in [floor_row, t] with band_mid(q) ==
// band_mid(t) that shares row t's page.
DYN_BR_HD int bwd_run_first(int t, double ratio, double inv_ratio, int floor_row, int log_r) {
  const int page_first = (t >> log_r) << log_r;
  return run_first_row(t, ratio, inv_ratio, page_first > floor_row ? page_first : floor_row);
}

}  // namespace dynband
