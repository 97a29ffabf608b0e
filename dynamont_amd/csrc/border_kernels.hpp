// border_kernels.hpp -- per-border posterior confidence (dyn_aligner_set_border_confidence): how much of the lattice's
// posterior mass for "segment n starts here" lies on the called border, and within W rows of it. Included by nt_kernels.hip
// and band_reads.hip (the phase behind traceback / mpost, while the read's lattice is still in its pages or arena) and by
// tests/device_math/border_confidence.hip, which runs border_window_sum on lattices the test writes itself.
//
// Definition (include/dynamont_mi.h). Output row j of an ok read is lattice column n = j + 1, the row
// of its M cell is r = segrow[j]; LPM(t, n) = (fM(t, n) + bM(t, n)) - Z (NT_aligner_api.cpp:213-224), -inf for every cell
// outside the reference's band window of row t (computeBounds, :90-108) and in row 0.
//   border_probability         exp(LPM(r, n))
//   border_window_probability  sum over t = max(1, r - W) .. min(T - 1, r + W) of exp(LPM(t, n)): fp64, ascending t, one
//                              __dadd_rn per term, not clamped (a value may exceed 1 by rounding)
// A cell accessor is "LPM(t, n) or -inf"; there is one per place a lattice lives:
//   BorderCellSeparate  separate layout (JOB_ALIGN): LPM rebuilt the way mpost does, from the float LPE and bE of (t-1, n-1),
//                       bE(t+1, n), the two emissions of column n, Zb and m1
//   BorderCellInplace   in-place layout (JOB_ALIGN_INPLACE): the float LPM half of the slot
//   BorderCellWide      band_reads.hip (diagonal window): lp[2 * cell] in the reference's band-column addressing
// EVERY accessor checks the band explicitly, for every cell it reads: a band slot is n mod 448, and a slot outside the band
// carries "no k-mer" values, another column's values or whatever the arena held before -- never something to rely on.
// Lane mapping: one lane per border (as mpost), the window rows in groups of eight whose loads are in flight together; no
// atomics, no LDS, no scratch memory, and no result depends on anything but the read's own lattice: the same bits run to run.
#pragma once

#include "nt_kernels.hpp"

namespace dynk {

constexpr int BC_MAX_WINDOW = 256;  // = DYN_BORDER_CONFIDENCE_MAX_WINDOW

// position of band slot s inside a stored row of the register sweeps (nt_kernels.hip: pos_of / row_pos)
__device__ __forceinline__ int border_row_pos(int s) {
  const int lane = s / CPL, j = s % CPL;
  return j < 6 ? (j >> 1) * 128 + lane * 2 + (j & 1) : 384 + lane;
}

// centre of the reference's band in lattice row t: size_t(t * RATIO) of NT_aligner_api.cpp:100, ratio = double(N) / double(T)
__device__ __forceinline__ int diagonal_centre(int t, double ratio) { return (int)__dmul_rn((double)t, ratio); }

// the band of a read: which cells (t, n) the reference's sweeps fill (computeBounds; rows 1 .. T-1, columns 1 .. N-1)
struct BorderBand {
  int T, N, bw;
  double ratio;
  __device__ __forceinline__ int start(int t) const { return diagonal_centre(t, ratio) - bw; }
  __device__ __forceinline__ bool holds(int t, int n) const {
    if (t < 1 || t >= T) return false;
    const int s = start(t);
    return n >= (s > 1 ? s : 1) && n < (s + 2 * bw + 1 < N ? s + 2 * bw + 1 : N);
  }
};

// ROW: lattice row -> row of the pool arrays (the wave's page table), callable as row(t) for t = 0 .. T.
// The accessors take no branch around their loads: whether the term exists is decided first, from t and n alone, and the
// addresses of a term that does not are clamped onto rows 0 .. T of this read's own lattice (all in its pages or arena), so
// that every load is in bounds, its value unused, and the loads of several window rows can be in flight at once
// (border_window_sum) -- a wave of the read queue is alone on its SIMD, and nothing else hides their latency.
__device__ __forceinline__ int border_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <class ROW>
struct BorderCellSeparate {
  BorderBand band;
  const float* __restrict__ lpe;   // [row][P] float LPE
  const double* __restrict__ bE;   // [row][P]
  const double* __restrict__ sg;   // the read's samples: sg[t - 1] belongs to row t
  const Emis* __restrict__ pr;     // the read's columns: entry n - 1 <-> column n
  double Zb, m1;
  ROW row;
  __device__ __forceinline__ double operator()(int t, int n) const {
    // the cell, its successor (t+1, n) (bM; row T-1 has none: bM = -inf there, :170) and its diagonal predecessor (t-1, n-1);
    // row 0 holds fE(0, 0) = 0 and nothing else (:120)
    const bool first = t == 1;
    const bool ok = band.holds(t, n) && band.holds(t + 1, n) && (first ? n == 1 : band.holds(t - 1, n - 1));
    const size_t pcell = (size_t)row(border_clamp(t - 1, 0, band.T)) * P + border_row_pos((n - 1) % P);
    const size_t ncell = (size_t)row(border_clamp(t + 1, 0, band.T)) * P + border_row_pos(n % P);
    const float l = lpe[pcell];
    const double b_prev = bE[pcell], b_next = bE[ncell];
    const double x_here = sg[border_clamp(t - 1, 0, band.T - 2)], x_next = sg[border_clamp(t, 0, band.T - 2)];
    const Emis em = pr[n - 1];
    // LPE = -inf: fE or bE of the predecessor is -inf. With bE(t-1, n-1) = -inf no path leaves M(t, n) either (the move into
    // it is one of that cell's two ways on), so LPM(t, n) = -inf both times -- and -inf - -inf must not be formed
    const bool dead = !first && l == -__builtin_huge_valf();
    const double fE_prev = first ? 0.0 : ((double)l - b_prev) + Zb;                              // :222 solved for fE
    const double fM = (fE_prev + dynmath::log_normal_pdf(x_here, em)) + m1;                      // :146
    const double bM = b_next + dynmath::log_normal_pdf(x_next, em);                              // :200
    return (ok && !dead) ? (fM + bM) - Zb : dynmath::NEG_INF;
  }
};

template <class ROW>
struct BorderCellInplace {
  BorderBand band;
  const float* __restrict__ lp;  // [row][P] (float LPM, float LPE)
  ROW row;
  __device__ __forceinline__ double operator()(int t, int n) const {
    const float l = lp[2 * ((size_t)row(border_clamp(t, 0, band.T)) * P + border_row_pos(n % P))];
    return band.holds(t, n) ? (double)l : dynmath::NEG_INF;
  }
};

struct BorderCellWide {
  BorderBand band;
  const float* __restrict__ lp;  // [t][2 bw + 3] (float LPM, float LPE), band column c = n - start_t + 1
  __device__ __forceinline__ double operator()(int t, int n) const {
    const int tc = border_clamp(t, 0, band.T - 1), B = 2 * band.bw + 3;
    const int c = border_clamp(n - band.start(tc) + 1, 0, B - 1);
    const float l = lp[2 * ((size_t)tc * (size_t)B + c)];
    return band.holds(t, n) ? (double)l : dynmath::NEG_INF;
  }
};

// one term of the sums: the mass of cell (t, n)
template <class CELL>
__device__ __forceinline__ double border_term(const CELL& cell, int t, int n) {
  const double l = cell(t, n);
  const double p = exp(l);
  return l == dynmath::NEG_INF ? 0.0 : p;
}

// the two columns of one border: column n, M row r, window W (1 .. BC_MAX_WINDOW), rows 1 .. T-1. The window is walked in
// groups of BC_GROUP rows: the terms of a group are evaluated side by side (their loads in flight together), then added in
// ascending row order. A row past the window's end contributes +0.0, which leaves every bit of the sum as it is (the sum is
// never -0.0), so the result is the one-add-per-term sum of the definition.
constexpr int BC_GROUP = 8;
template <class CELL>
__device__ __forceinline__ void border_window_sum(const CELL& cell, int n, int r, int T, int W, double& at_border, double& in_window) {
  const int t_lo = r - W > 1 ? r - W : 1, t_hi = r + W < T - 1 ? r + W : T - 1;
  double sum = 0.0, here = 0.0;
#pragma unroll 1
  for (int t = t_lo; t <= t_hi; t += BC_GROUP) {
    double p[BC_GROUP];
#pragma unroll
    for (int u = 0; u < BC_GROUP; ++u) {
      const double v = border_term(cell, t + u, n);
      p[u] = t + u <= t_hi ? v : 0.0;
    }
#pragma unroll
    for (int u = 0; u < BC_GROUP; ++u) {
      here = t + u == r ? p[u] : here;
      sum = __dadd_rn(sum, p[u]);
    }
  }
  at_border = here;
  in_window = sum;
}

// the phase: every border of the read, one per thread of the `n_threads` that call this (tid = 0 .. n_threads-1)
template <class CELL>
__device__ __forceinline__ void border_confidence_read(const CELL& cell, const ReadDesc& rd, const uint32_t* __restrict__ segrow,
                                                       double* __restrict__ border_p, double* __restrict__ window_p, int W,
                                                       int tid, int n_threads) {
  const int T = (int)rd.T, N = (int)rd.N;
  for (int n = 1 + tid; n < N; n += n_threads) {
    const int r = (int)segrow[rd.seg_off + n - 1];
    double here, sum;
    border_window_sum(cell, n, r, T, W, here, sum);
    border_p[rd.seg_off + n - 1] = here;
    window_p[rd.seg_off + n - 1] = sum;
  }
}

}  // namespace dynk
