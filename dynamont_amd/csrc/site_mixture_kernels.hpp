// site_mixture_kernels.hpp -- a two-component Gaussian mixture fitted per site pair to the per-site level histograms by EM
// (dyn_aligner_site_mixture). Included by site_summary.hip (launch_site_mixture) and by tests/device_math/site_mixture.hip, which
// runs the kernel on tables the test uploads and compares every output, doubles by their bits, with a restatement in Python floats
// (tests/site_mixture_cases.py, tests/test_gpu_site_mixture.py).
//
// Definition. Pair i of a window of `count` pairs: A = site_lo + i, B = other_lo + i; the single-sample
// form has no B (all of B's counters count as 0). a[e], b[e] their Bc = bins + 2 level counters (e = 0 under, e = Bc - 1 over); the
// dwell counters are not used. Every floating-point operation is ONE IEEE fp64 operation in the order written (__dadd_rn, __dmul_rn,
// __ddiv_rn, __dsqrt_rn; the unit is built with -ffp-contract=off); exp is exp_strict_vec (dp_math_strict.hpp), every argument <= 0.
//   constants (host)  w = (hi - lo) / bins, vfloor = (w * w) / 12, tol_mu = tol * w, tol_pi = tol
//   x[e] = lo + ((double)e - 0.5) * w
//   c[e] = (double)a[e] + (double)b[e] for 1 <= e <= bins, c[0] = c[Bc - 1] = 0 (under and over take no part in the fit)
//   n_a, n_b  the sums of the in-range counters of each side, out_a, out_b under + over (uint32, mod 2^32)
//   gsum(t)   lane l of the group of G lanes owns e = r * G + l; its partial starts at +0.0 and adds t[e] in rising r (an index
//             >= Bc adds 0.0); then for m = 1, 2, 4, .. < G every lane adds its __shfl_xor(.., m, G) partner's value. fp addition
//             commutes: all lanes of a group end with the same bits.
//   start     n = gsum(c); status 1 if n < min_n. m = gsum(c * x) / n, v = gsum(c * ((x - m) * (x - m))) / n; status 1 if not
//             v > vfloor. sd = sqrt(v), mu = (m - sd, m + sd), var = (v, v), pi = (0.5, 0.5)
//   E-step    A_k = pi_k / sqrt(var_k); d_k = x - mu_k, q_k = -0.5 * ((d_k * d_k) / var_k), qm = q_1 > q_0 ? q_1 : q_0,
//             p_k = A_k * exp(q_k - qm), s = p_0 + p_1, g_k = p_k / s
//   M-step    round it = 1 .. max_iters: t_k = c * g_k, N_k = gsum(t_k). N_0 < 1 or N_1 < 1: status 3, the parameters stay, iters =
//             it - 1. Else mu'_k = gsum(t_k * x) / N_k, var'_k = max(gsum(t_k * ((x - mu'_k) * (x - mu'_k))) / N_k, vfloor),
//             pi'_k = N_k / (N_0 + N_1); adopted; status 0 and stop when max_k |mu'_k - mu_k| <= tol_mu and |pi'_1 - pi_1| <= tol_pi.
//             max_iters rounds without that: status 2.
//   shares    one more E-step with the FINAL parameters: r_a = gsum((double)a * g_1), r_b = gsum((double)b * g_1), under and over
//             excluded
//   labels    mu_0 > mu_1 at the end: the components are exchanged in every output, the g of the shares included
//   outputs   pi1, mu0, mu1, var0, var1, r_a, r_b (float64; NaN 0x7FF8000000000000 at status 1, iters = 0 there), n_a, n_b, out_a,
//             out_b, iters, status (uint32)
// Of the two exponentials of a counter one has the argument +0.0 and exp_strict(+0.0) is 1.0 exactly (tests/test_site_mixture_host.py
// checks that): the kernel evaluates the other one and selects 1.0.
//
// The hazard: groups that share a wave stop after different numbers of rounds, and every reduction is a shuffle. The trip count is
// wave-uniform (while any live group of the WAVE is unfinished, up to max_iters); a finished, refused or dead group keeps its state
// by selects, so every shuffle runs with all lanes of the wave active.
//
// Footprint: 256 threads, 2 KB of LDS (the strict exp table, staged once per block from the engine's device copy: the E-step's
// lookups are lane-divergent), no atomics, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dp_math_strict.hpp"
#include "nt_kernels.hpp"

namespace dynk {

template <int G, int ROUNDS>
__device__ __forceinline__ double sm_gsum(const double (&t)[ROUNDS], const bool (&in)[ROUNDS]) {
  double s = 0.0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) s = __dadd_rn(s, in[r] ? t[r] : 0.0);  // an index >= Bc adds 0.0
#pragma unroll
  for (int m = 1; m < G; m <<= 1) s = __dadd_rn(s, __shfl_xor(s, m, G));
  return s;
}

template <int G>
__device__ __forceinline__ uint32_t sm_isum(uint32_t v) {
#pragma unroll
  for (int m = 1; m < G; m <<= 1) v += __shfl_xor(v, m, G);
  return v;
}

struct SmParams {
  double mu0, mu1, var0, var1, pi0, pi1;
};

// the E-step of a lane's ROUNDS counters (an index >= Bc, in[r] false, gets g = 0; gsum skips it anyway)
template <int ROUNDS>
__device__ __forceinline__ void sm_estep(const SmParams& P, const double (&x)[ROUNDS], const bool (&in)[ROUNDS], const uint64_t* tab,
                                         double (&g0)[ROUNDS], double (&g1)[ROUNDS]) {
  const double A0 = __ddiv_rn(P.pi0, __dsqrt_rn(P.var0)), A1 = __ddiv_rn(P.pi1, __dsqrt_rn(P.var1));
  double arg[ROUNDS], ex[ROUNDS];
  bool up[ROUNDS];  // q_1 > q_0: qm = q_1
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const double d0 = __dadd_rn(x[r], -P.mu0), d1 = __dadd_rn(x[r], -P.mu1);
    const double q0 = __dmul_rn(-0.5, __ddiv_rn(__dmul_rn(d0, d0), P.var0));
    const double q1 = __dmul_rn(-0.5, __ddiv_rn(__dmul_rn(d1, d1), P.var1));
    up[r] = q1 > q0;
    arg[r] = up[r] ? __dadd_rn(q0, -q1) : __dadd_rn(q1, -q0);
  }
  dynmath::exp_strict_vec<ROUNDS>(arg, ex, tab);
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const double p0 = __dmul_rn(A0, up[r] ? ex[r] : 1.0), p1 = __dmul_rn(A1, up[r] ? 1.0 : ex[r]);
    const double s = __dadd_rn(p0, p1);
    g0[r] = in[r] ? __ddiv_rn(p0, s) : 0.0;
    g1[r] = in[r] ? __ddiv_rn(p1, s) : 0.0;
  }
}

// A group of G = min(64, the power of two >= Bc, at least 4) lanes owns one pair: lane l holds the counters l, l + G, ... of both
// sites (as doubles: they are exact), so a group's loads are neighbouring words; ROUNDS = ceil(Bc / G) rounds, at most four (Bc <=
// 256) and one for G < 64. (k_site_compare always runs four rounds at G = 64; here a round costs an exponential and a dozen
// divisions per EM round, and a round past Bc only adds 0.0 to partials that are never -0.0: leaving it out changes no bit.) Lanes
// of pairs outside the window load nothing and store nothing. The two windows may lie anywhere in the table, in either order, and
// may overlap: nothing is written to the table. Block of 256.
template <int G, int ROUNDS>
__global__ __launch_bounds__(256) void k_site_mixture(SiteMixture sm) {
  __shared__ uint64_t s_exp[dynmath::STRICT_EXP_WORDS];
  for (int i = threadIdx.x; i < dynmath::STRICT_EXP_WORDS; i += 256) s_exp[i] = sm.exp_tab[i];
  __syncthreads();
  const uint32_t B = sm.bins + 2u, H = B + (uint32_t)SH_DWELL_BINS;
  const int l = (int)(threadIdx.x & 63u) & (G - 1);
  const uint64_t pair = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / (uint32_t)G;
  const bool live = pair < sm.count;
  const unsigned int* __restrict__ ha = sm.hist_a + pair * H;
  const unsigned int* __restrict__ hb = sm.hist_b ? sm.hist_b + pair * H : nullptr;
  double x[ROUNDS], c[ROUNDS], fa[ROUNDS], fb[ROUNDS], t[ROUNDS], u[ROUNDS];
  bool in[ROUNDS];
  uint32_t n_a = 0, n_b = 0, out_a = 0, out_b = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const uint32_t e = (uint32_t)(r * G + l);
    in[r] = e < B;
    const bool ld = live && in[r];
    const uint32_t va = ld ? ha[e] : 0u, vb = (ld && hb) ? hb[e] : 0u;
    const bool fit = e >= 1u && e <= sm.bins;
    n_a += fit ? va : 0u;
    n_b += fit ? vb : 0u;
    out_a += fit ? 0u : va;
    out_b += fit ? 0u : vb;
    fa[r] = fit ? (double)va : 0.0;
    fb[r] = fit ? (double)vb : 0.0;
    c[r] = __dadd_rn(fa[r], fb[r]);
    x[r] = __dadd_rn(sm.lo, __dmul_rn(__dadd_rn((double)e, -0.5), sm.w));
  }
  n_a = sm_isum<G>(n_a);
  n_b = sm_isum<G>(n_b);
  out_a = sm_isum<G>(out_a);
  out_b = sm_isum<G>(out_b);
  // start
  const double n = sm_gsum<G, ROUNDS>(c, in);
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) t[r] = in[r] ? __dmul_rn(c[r], x[r]) : 0.0;
  const double m = __ddiv_rn(sm_gsum<G, ROUNDS>(t, in), n);
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const double d = __dadd_rn(x[r], -m);
    t[r] = in[r] ? __dmul_rn(c[r], __dmul_rn(d, d)) : 0.0;
  }
  const double v = __ddiv_rn(sm_gsum<G, ROUNDS>(t, in), n);
  const bool fitted = !(n < (double)sm.min_n) && v > sm.vfloor;
  const double sd = __dsqrt_rn(v);
  SmParams P{__dadd_rn(m, -sd), __dadd_rn(m, sd), v, v, 0.5, 0.5};
  uint32_t status = fitted ? 2u : 1u, iters = 0;
  bool active = live && fitted;
  double g0[ROUNDS], g1[ROUNDS];
  for (uint32_t it = 1; it <= sm.max_iters; ++it) {
    if (__ballot(active) == 0ull) break;  // wave-uniform: every lane of the wave runs every shuffle below
    sm_estep<ROUNDS>(P, x, in, s_exp, g0, g1);
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      t[r] = __dmul_rn(c[r], g0[r]);
      u[r] = __dmul_rn(c[r], g1[r]);
    }
    const double N0 = sm_gsum<G, ROUNDS>(t, in), N1 = sm_gsum<G, ROUNDS>(u, in);
    const bool collapsed = N0 < 1.0 || N1 < 1.0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      g0[r] = __dmul_rn(t[r], x[r]);
      g1[r] = __dmul_rn(u[r], x[r]);
    }
    const double nm0 = __ddiv_rn(sm_gsum<G, ROUNDS>(g0, in), N0), nm1 = __ddiv_rn(sm_gsum<G, ROUNDS>(g1, in), N1);
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const double d0 = __dadd_rn(x[r], -nm0), d1 = __dadd_rn(x[r], -nm1);
      g0[r] = __dmul_rn(t[r], __dmul_rn(d0, d0));
      g1[r] = __dmul_rn(u[r], __dmul_rn(d1, d1));
    }
    const double q0 = __ddiv_rn(sm_gsum<G, ROUNDS>(g0, in), N0), q1 = __ddiv_rn(sm_gsum<G, ROUNDS>(g1, in), N1);
    const double nv0 = sm.vfloor > q0 ? sm.vfloor : q0, nv1 = sm.vfloor > q1 ? sm.vfloor : q1;
    const double tot = __dadd_rn(N0, N1);
    const double np0 = __ddiv_rn(N0, tot), np1 = __ddiv_rn(N1, tot);
    const double dm0 = fabs(__dadd_rn(nm0, -P.mu0)), dm1 = fabs(__dadd_rn(nm1, -P.mu1));
    const double dm = dm1 > dm0 ? dm1 : dm0, dp = fabs(__dadd_rn(np1, -P.pi1));
    const bool adopt = active && !collapsed;
    const bool done = dm <= sm.tol_mu && dp <= sm.tol_pi;
    P.mu0 = adopt ? nm0 : P.mu0;
    P.mu1 = adopt ? nm1 : P.mu1;
    P.var0 = adopt ? nv0 : P.var0;
    P.var1 = adopt ? nv1 : P.var1;
    P.pi0 = adopt ? np0 : P.pi0;
    P.pi1 = adopt ? np1 : P.pi1;
    iters = adopt ? it : iters;
    status = active ? (collapsed ? 3u : (done ? 0u : 2u)) : status;
    active = adopt && !done;
  }
  // shares, with the final parameters; labels
  sm_estep<ROUNDS>(P, x, in, s_exp, g0, g1);
  const bool swap = P.mu0 > P.mu1;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const double g = swap ? g0[r] : g1[r];
    t[r] = __dmul_rn(fa[r], g);
    u[r] = __dmul_rn(fb[r], g);
  }
  const double r_a = sm_gsum<G, ROUNDS>(t, in), r_b = sm_gsum<G, ROUNDS>(u, in);
  if (live && l == 0) {
    const uint64_t cnt = sm.count;
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const bool none = status == 1u;
    double* __restrict__ o = sm.out;
    o[pair] = none ? nan : (swap ? P.pi0 : P.pi1);
    o[cnt + pair] = none ? nan : (swap ? P.mu1 : P.mu0);
    o[2 * cnt + pair] = none ? nan : (swap ? P.mu0 : P.mu1);
    o[3 * cnt + pair] = none ? nan : (swap ? P.var1 : P.var0);
    o[4 * cnt + pair] = none ? nan : (swap ? P.var0 : P.var1);
    o[5 * cnt + pair] = none ? nan : r_a;
    o[6 * cnt + pair] = none ? nan : r_b;
    uint32_t* __restrict__ o32 = reinterpret_cast<uint32_t*>(o + 7 * cnt);
    o32[pair] = n_a;
    o32[cnt + pair] = n_b;
    o32[2 * cnt + pair] = out_a;
    o32[3 * cnt + pair] = out_b;
    o32[4 * cnt + pair] = iters;
    o32[5 * cnt + pair] = status;
  }
}

inline void launch_site_mixture_kernel(const SiteMixture& sm, hipStream_t s) {
  if (!sm.hist_a || !sm.exp_tab || !sm.out || sm.count == 0 || sm.bins < 2 || sm.bins > (uint32_t)SH_BINS_MAX || sm.max_iters < 1) return;
  const uint32_t B = sm.bins + 2u;
  uint32_t G = 4;
  while (G < B && G < 64) G <<= 1;
  const unsigned blocks = (unsigned)(((uint64_t)sm.count * G + 255u) / 256u);
  switch (G) {
    case 4: hipLaunchKernelGGL((k_site_mixture<4, 1>), dim3(blocks), dim3(256), 0, s, sm); break;
    case 8: hipLaunchKernelGGL((k_site_mixture<8, 1>), dim3(blocks), dim3(256), 0, s, sm); break;
    case 16: hipLaunchKernelGGL((k_site_mixture<16, 1>), dim3(blocks), dim3(256), 0, s, sm); break;
    case 32: hipLaunchKernelGGL((k_site_mixture<32, 1>), dim3(blocks), dim3(256), 0, s, sm); break;
    default:
      switch ((B + 63u) / 64u) {  // the rounds a group of 64 needs
        case 1: hipLaunchKernelGGL((k_site_mixture<64, 1>), dim3(blocks), dim3(256), 0, s, sm); break;
        case 2: hipLaunchKernelGGL((k_site_mixture<64, 2>), dim3(blocks), dim3(256), 0, s, sm); break;
        case 3: hipLaunchKernelGGL((k_site_mixture<64, 3>), dim3(blocks), dim3(256), 0, s, sm); break;
        default: hipLaunchKernelGGL((k_site_mixture<64, 4>), dim3(blocks), dim3(256), 0, s, sm); break;
      }
      break;
  }
}

}  // namespace dynk
