// exact_sum_kernels.hpp -- what the run-wide summaries share (kmer_summary_kernels.hpp: per k-mer; site_summary_kernels.hpp: per
// caller-supplied site): the chunked fp64 sums of event_stats.hip over one segment, an integer-valued double as a 128-bit
// two's complement integer, and the 128-bit atomic add in two 64-bit limbs. Inline device functions only: any number of
// translation units may include this file (the two kernel headers define ordinary kernels, one translation unit each).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dynk {

constexpr int XS_CHUNK = 64;
constexpr double XS_SCALE = 1099511627776.0;       // 2^40: the fixed point of every summed value
constexpr double XS_TWO64 = 18446744073709551616.0;

// chunks of 64 from the segment's first sample, each left to right, the chunk sums left to right; one IEEE fp64 operation
// each, no contraction: S1 of x and S2 of __dmul_rn(x, x)
__device__ __forceinline__ void xs_chunked_sums(const double* __restrict__ x, int L, double& s1, double& s2) {
  double a1 = 0.0, a2 = 0.0;
  for (int c0 = 0; c0 < L; c0 += XS_CHUNK) {
    const int c1 = min(c0 + XS_CHUNK, L);
    double v = x[c0];
    double c1s = v, c2s = __dmul_rn(v, v);
    for (int j = c0 + 1; j < c1; ++j) {
      v = x[j];
      c1s = __dadd_rn(c1s, v);
      c2s = __dadd_rn(c2s, __dmul_rn(v, v));
    }
    a1 = c0 == 0 ? c1s : __dadd_rn(a1, c1s);
    a2 = c0 == 0 ? c2s : __dadd_rn(a2, c2s);
  }
  s1 = a1;
  s2 = a2;
}

// S1 alone, the same additions in the same order
__device__ __forceinline__ double xs_chunked_sum(const double* __restrict__ x, int L) {
  double a1 = 0.0;
  for (int c0 = 0; c0 < L; c0 += XS_CHUNK) {
    const int c1 = min(c0 + XS_CHUNK, L);
    double c1s = x[c0];
    for (int j = c0 + 1; j < c1; ++j) c1s = __dadd_rn(c1s, x[j]);
    a1 = c0 == 0 ? c1s : __dadd_rn(a1, c1s);
  }
  return a1;
}

// an integer-valued double of magnitude below 2^116 as a 128-bit two's complement integer: the significand shifted by the
// exponent (__double2ll_rn covers |v| < 2^63 only; the summed values reach 2^104)
__device__ __forceinline__ void xs_to_i128(double v, unsigned long long& lo, unsigned long long& hi) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  const int e = (int)((bits >> 52) & 0x7ffu);
  lo = 0;
  hi = 0;
  if (e == 0) return;  // +-0 (an integer-valued double is never denormal)
  const unsigned long long m = (bits & 0x000fffffffffffffull) | 0x0010000000000000ull;
  const int sh = e - 1075;  // v = m * 2^sh
  if (sh < 0) {
    lo = m >> (-sh);  // |v| >= 1: sh >= -52, and the bits shifted out are zero
  } else if (sh == 0) {
    lo = m;
  } else if (sh < 64) {
    lo = m << sh;
    hi = m >> (64 - sh);
  } else {
    hi = m << (sh - 64);  // sh <= 63 + 52 for every value the definitions keep
  }
  if (bits >> 63) {
    lo = ~lo + 1ull;
    hi = ~hi + (lo == 0 ? 1ull : 0ull);
  }
}

// cell += (hi:lo) mod 2^128: the low limb first, the carry from the value it replaced
__device__ __forceinline__ void xs_add128(unsigned long long* cell, unsigned long long lo, unsigned long long hi) {
  unsigned long long up = hi;
  if (lo) {
    const unsigned long long old = atomicAdd(cell, lo);
    up += (old + lo < old) ? 1ull : 0ull;
  }
  if (up) atomicAdd(cell + 1, up);
}

__device__ __forceinline__ unsigned long long xs_wave_sum(unsigned long long v) {
  for (int d = warpSize >> 1; d > 0; d >>= 1) v += __shfl_down(v, d);
  return v;
}

}  // namespace dynk
