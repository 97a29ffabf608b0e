// dp_cell.hpp -- the device-only part of one lattice cell's arithmetic: the sweeps' arithmetic flavours, their emission, the
// wave-level second half of the certified logPlus and the places of the two exponential tables behind the softplus nodes.
// Included by nt_kernels.hip (the sweeps) and by tests/device_math/cell_math.hip, which runs each piece on its own and
// compares its bits with the host build of dp_math.hpp / dp_math_strict.hpp (tests/test_gpu_cell_math.py).
#pragma once

#include "nt_kernels.hpp"

#include "dp_math_strict.hpp"

namespace dynk {

using dynmath::EmisV;
using dynmath::log_normal_pdf_vec;
using dynmath::SoftplusNode;
using dynmath::SoftplusLookup;
using dynmath::SP_NODES;

// Arithmetic flavours of the sweeps.
//  ARITH_DEFAULT  dp_math.hpp: 5-operation emission, table softplus (<= 1 ulp from glibc)
//  ARITH_STRICT   dp_math_strict.hpp, "certified arithmetic": the reference's bits. The emission's quotient is formed exactly
//                 from 1/stdev and stdev (one multiplication, four FMAs, no division); a logPlus is the table softplus plus
//                 a rounding certificate (5 operations), and only the registers that hold an AMBIGUOUS sum -- one whose
//                 rounding could depend on the last bits of glibc's log1p(exp()) -- are recomputed with the restated glibc
//  ARITH_FOLDED   train() only (its backward sweep; the forward sweep is the posterior chain): emission ln K - u^2 in three
//                 operations, softplus polynomial of degree 3. No integer decision hangs on the last bits there,
//                 unlike in the align sweeps: train()'s outputs are sums of posteriors
constexpr int ARITH_DEFAULT = 0, ARITH_STRICT = 1, ARITH_FOLDED = 2;

template <int ARITH>
__device__ __forceinline__ void set_emis(EmisV<CPL>& p, int j, const Emis& e) {
  p.set(j, e);
  if (ARITH == ARITH_FOLDED) {  // train(): ln P = ln K - u^2, u = (x - mu) c, c = 1/(stdev sqrt 2) -- three operations, one fused
    p.inv_stdev[j] = e.inv_stdev * 0x1.6a09e667f3bcdp-1;
    p.neg_log_stdev[j] = e.neg_log_stdev - dynmath::HALF_LOG_2PI;
  }
}

// stdev: ARITH_STRICT only (the divisor of the reference's quotient, beside its reciprocal in p)
// y_lo: ARITH_STRICT only (the low part of 1/stdev: the exact quotient in four operations, dp_math_strict.hpp; -DDYN_QUOT5 keeps
// round 4's five)
template <int ARITH, int NS>
__device__ __forceinline__ void emission_vec(double x, const EmisV<CPL>& p, const double (&stdev)[NS], const double (&y_lo)[NS], double (&out)[CPL]) {
  if constexpr (ARITH == ARITH_STRICT) {
    static_assert(NS == CPL, "strict emission needs every cell's stdev");
#ifdef DYN_QUOT5
    dynmath::log_normal_pdf_cert_vec<CPL>(x, p, stdev, out);
#else
    dynmath::log_normal_pdf_cert4_vec<CPL>(x, p, stdev, y_lo, out);
#endif
  } else if constexpr (ARITH == ARITH_FOLDED) {
    double u[CPL];
    // The difference FIRST: u = fma(x, c, -RN(mu c)) saves this operation but carries the rounding of mu c, an error that
    // grows with |mu| / stdev (5.1 ulp of the terms of the result against 3.4 now, tests/test_gpu_cell_math.py).
#pragma unroll
    for (int j = 0; j < CPL; ++j) u[j] = x - p.mean[j];
#pragma unroll
    for (int j = 0; j < CPL; ++j) u[j] = u[j] * p.inv_stdev[j];
#pragma unroll
    for (int j = 0; j < CPL; ++j) out[j] = dynmath::fma_(-u[j], u[j], p.neg_log_stdev[j]);
  } else {
    log_normal_pdf_vec<CPL>(x, p, out);
  }
}

// Second half of a certified logPlus (dp_math_strict.hpp): out = the reference's sum bit for bit. The registers in which
// some lane's certificate failed (a rounding boundary inside the interval: ~1e-4 of the cells of a 20 k-sample read,
// profiles/r04/cert_ambiguity.json) are recomputed with the restated glibc -- for all 64 lanes of that register: where the
// certificate held, the restated value IS the certified one.

__device__ __forceinline__ void log_plus_finish_certified(const SoftplusLookup<CPL>& L, double (&out)[CPL], const uint64_t* exp_tab,
                                                          uint32_t& fallbacks) {
  double hi[CPL];
  dynmath::log_plus_finish_cert<CPL>(L, out, hi);
  // One branch per row, not one test per register: the seven comparison masks are OR-ed (7 v_cmp + 6 s_or_b64, where the
  // per-register form took a compare, a select and an OR of SALU each), and which registers hold the ambiguous sums is only
  // worked out on the rare path.
#ifdef DYN_EXP_NO_CERT_BRANCH  // development (WRONG results): what the ambiguity test and its branch cost the certified rows
  (void)hi; (void)exp_tab; (void)fallbacks;
  return;
#endif
  uint64_t any_amb = 0;
#pragma unroll
  for (int j = 0; j < CPL; ++j) any_amb |= __ballot(out[j] != hi[j]);
  if (__builtin_expect(any_amb != 0, 0)) {
#ifdef DYN_EXP_NO_CERT_FALLBACK  // development (WRONG results): the test and the branch, but no recomputation
    ++fallbacks;
    return;
#endif
    unsigned amb = 0;  // wave-uniform: bit j = some lane's certificate failed in register j
#pragma unroll
    for (int j = 0; j < CPL; ++j) amb |= __any(out[j] != hi[j]) ? 1u << j : 0u;
    // ONE copy of the restated glibc (M = 1) for whichever registers need it: the operands are picked by the uniform
    // register number (a select chain: ~30 instructions per pass, next to ~130 of the restatement itself). Unrolled by
    // register, the seven copies cost the hot loop 100 spilled VGPRs.
#pragma unroll 1
    for (int j = 0; j < CPL; ++j) {
      if (!((amb >> j) & 1u)) continue;
      ++fallbacks;
      double hj = L.hi[0], dj = L.diff[0];
#pragma unroll
      for (int k = 1; k < CPL; ++k) {
        hj = (j == k) ? L.hi[k] : hj;
        dj = (j == k) ? L.diff[k] : dj;
      }
      const double v = dynmath::log_plus_strict_from(hj, dj, exp_tab);
#pragma unroll
      for (int k = 0; k < CPL; ++k) out[k] = (j == k) ? v : out[k];
    }
  }
}

__device__ __forceinline__ const uint64_t* strict_tab(const SoftplusNode* s_tab) {
  return reinterpret_cast<const uint64_t*>(s_tab + SP_NODES + dynmath::EXP128_NODES);
}
__device__ __forceinline__ const double* exp128_tab(const SoftplusNode* s_tab) {
  return reinterpret_cast<const double*>(s_tab + SP_NODES);
}

}  // namespace dynk
