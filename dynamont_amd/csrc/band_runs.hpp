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

}  // namespace dynband
