// auto_guide_kernels.hpp -- the self-made guide (dyn_batch_auto_guide, auto_guide.hip): a forward max-plus (Viterbi) sweep over
// the read's lattice whose window follows the row's best cell, and which writes that centre out as the read's guide -- one int32
// per signal sample, the layout dyn_batch_set_guide takes. One sweep, two rows (vE, vM), no arena, no exp table, no logPlus.
//
// Definition, fp64. T = samples + 1 rows, N = k-mers + 1 columns,
// score(t, n) = log_normal_pdf_strict(signal[t - 1], par[n - 1]), m1 / e2 the handle's log transitions, hw the half width.
//   row 0   vE[0] = 0, everything else -inf; c = 0; the previous window is [0, 1)
//   row t   s(n) = (vM[n] < vE[n]) ? vE[n] : vM[n] over the previous row's window
//           a    = the lowest n whose s(n) is maximal, compared with '>' (a NaN never wins); a = c when no s(n) exceeds -inf
//           lo   = max(0, N - 1 - (T - 1 - t) / 2), hi = min(N - 1, (t + 1) / 2)          (a column takes two rows)
//           c    = min(max(c, a, lo), hi); guide[t - 1] = c
//           the cells of row t are n in [max(c - hw, 1), min(c + hw + 1, N)):
//           vM'[n] = (vE[n - 1] + score) + m1
//           vE'[n] = max((vM[n] + score) + 0.0, (vE[n] + score) + e2)                     (outside the previous window: -inf)
// The guide never decreases, lies in [0, N - 1] and connects the corners (lo == hi == N - 1 in the last row of a read with
// T - 1 >= 2 (N - 1)). A non-finite sample makes every later s(n) NaN or -inf: the centre then follows lo alone, the guide is
// still a valid one, and the read fails the guided job's own Z check.
//
// The arithmetic of a cell, the argmax rule and the centre update are the DYN_HD functions below; auto_guide_sequential is the
// same text walked by one thread, and its g++ build (-ffp-contract=off) is the yardstick of the kernel
// (tests/test_auto_guide_host.py, tests/test_gpu_auto_guide.py).
#pragma once

#include <cstdint>

#include "dp_math_strict.hpp"

namespace dynk {

constexpr int AG_NONE = 0x7fffffff;  // "no cell has entered the argmax yet"

// vM', vE' of one cell from the previous row's vE[n - 1], vE[n], vM[n]
DYN_HD void ag_cell(double pE_left, double pE, double pM, double score, double m1, double e2, double& vE, double& vM) {
  vM = (pE_left + score) + m1;
  const double x = (pM + score) + 0.0, y = (pE + score) + e2;
  vE = (x < y) ? y : x;
}

DYN_HD double ag_s(double vE, double vM) { return (vM < vE) ? vE : vM; }

// (bv, bn) <- the better of (bv, bn) and (v, n): the larger value, of equal values the lower column. Symmetric in its two
// candidates, so a tree of merges gives what the ascending scan gives.
DYN_HD void ag_merge(double& bv, int& bn, double v, int n) {
  if (v > bv || (v == bv && n < bn)) {
    bv = v;
    bn = n;
  }
}

// a cell enters the argmax only with a value above -inf: neither a NaN nor an empty cell ever wins
DYN_HD void ag_take(double& bv, int& bn, double s, int n) {
  if (s > -__builtin_inf()) ag_merge(bv, bn, s, n);
}

// the centre of row t from the previous centre c and the previous row's argmax a (a < 0: none)
DYN_HD int ag_centre(int c, int a, int t, int T, int N) {
  const int lo_raw = (N - 1) - (T - 1 - t) / 2, lo = lo_raw > 0 ? lo_raw : 0;
  const int hi_raw = (t + 1) / 2, hi = hi_raw < N - 1 ? hi_raw : N - 1;
  int m = c;
  if (a > m) m = a;
  if (lo > m) m = lo;
  if (m > hi) m = hi;
  return m;
}

// One read, one thread, whole rows in absolute columns (vE / vM / nE / nM: N doubles each of the caller's). guide: T - 1 entries.
inline void auto_guide_sequential(int T, int N, int hw, const double* sig, const dynmath::Emis* par, double m1, double e2,
                                  int32_t* guide, double* vE, double* vM, double* nE, double* nM) {
  const double NEG = -__builtin_inf();
  for (int n = 0; n < N; ++n) vE[n] = vM[n] = NEG;
  vE[0] = 0.0;
  int c = 0, w_lo = 0, w_hi = 1;
  for (int t = 1; t < T; ++t) {
    double bv = NEG;
    int bn = AG_NONE;
    for (int n = w_lo; n < w_hi; ++n) ag_take(bv, bn, ag_s(vE[n], vM[n]), n);
    c = ag_centre(c, bn == AG_NONE ? -1 : bn, t, T, N);
    guide[t - 1] = (int32_t)c;
    const int lo = c - hw > 1 ? c - hw : 1, hi = c + hw + 1 < N ? c + hw + 1 : N;
    auto prev = [&](const double* row, int n) { return (n >= w_lo && n < w_hi) ? row[n] : NEG; };
    const double x = sig[t - 1];
    for (int n = lo; n < hi; ++n)
      ag_cell(prev(vE, n - 1), prev(vE, n), prev(vM, n), dynmath::log_normal_pdf_strict(x, par[n - 1]), m1, e2, nE[n], nM[n]);
    for (int n = lo; n < hi; ++n) {
      vE[n] = nE[n];
      vM[n] = nM[n];
    }
    w_lo = lo;
    w_hi = hi > lo ? hi : lo;
  }
}

}  // namespace dynk

// ---- launch interface (DYN_AUTO_GUIDE_MATH_ONLY: the arithmetic above alone, for a plain host build without the HIP headers) ----
#if !defined(DYN_AUTO_GUIDE_MATH_ONLY)
#include "nt_kernels.hpp"

namespace dynk {

struct AutoGuideArgs {
  const ReadDesc* descs;  // the reads to guide: T, N, sig_off, par_off are read
  int n_reads;
  int bw;                 // half width, 1 .. WIDE_MAX_HALF_BAND
  const double* sig;
  const Emis* par;
  int32_t* guide;         // [samples of the batch]: T - 1 entries per read at ReadDesc::sig_off
  uint32_t* head;         // queue head (cleared by launch_auto_guide)
  double m1, e2;
  // the guide rescue (dyn_aligner_set_guide_rescue): the reads to guide are descs[active[0 .. *n_active)], list and length written
  // on the device by launch_rescue_select. Null: every descriptor
  const uint32_t* active = nullptr;
  const uint32_t* n_active = nullptr;
};

// the most workgroups per compute unit worth launching at this half width
int auto_guide_groups_per_cu(int bw);
// k_auto_guide over a.descs with n_groups workgroups that take reads off a queue. Returns what raising the dynamic-LDS limit
// (windows above 48 KiB of rows) or the launch reported.
hipError_t launch_auto_guide(const AutoGuideArgs& a, int n_groups, hipStream_t s);

}  // namespace dynk
#endif
