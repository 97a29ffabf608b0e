// site_compare_kernels.hpp -- two samples in one per-site table: the comparison of two windows of the per-site histograms
// (dyn_aligner_site_compare) and the exact add of host columns into the table and its counters (dyn_aligner_site_summary_add).
// Included by site_summary.hip (launch_site_compare, launch_site_add) and by tests/device_math/site_compare.hip, which runs both
// kernels on arrays the test uploads and compares every output integer with a Python-int restatement
// (tests/test_gpu_site_compare.py).
//
// Definition of the comparison. Pair i of a window of `count` pairs: A = site_lo + i, B = other_lo + i.
// a[e], b[e] their Bc = bins + 2 level counters, PA[e], PB[e] the inclusive prefix sums (uint32: fewer than 2^32 rows per site is
// the defined domain, as for the quantiles), nA = PA[Bc - 1], nB = PB[Bc - 1]. Per counter
//   x[e] = (uint64)PA[e] * nB,  y[e] = (uint64)PB[e] * nA,  d[e] = x[e] > y[e] ? x[e] - y[e] : y[e] - x[e]
// (a product of two uint32 fits a uint64). Per pair
//   level_num   max_e d[e]
//   level_at    the SMALLEST e with d[e] == level_num
//   level_side  +1 if x[at] > y[at] (A's distribution function is ahead: A's levels are lower), -1 if x[at] < y[at], 0 when
//               level_num == 0
//   nA == 0 or nB == 0: level_num = 0, level_at = SC_NO_AT (0xFFFFFFFF), level_side = 0
// and the same three over the 16 dwell counters with the dwell counters' own totals (dwell_num, dwell_at, dwell_side); n_a = nA,
// n_b = nB. The binned Kolmogorov-Smirnov statistic is D = level_num / (nA * nB), formed on the host. Every output is an integer
// and integer adds, products and maxima do not depend on order: the same bits on every launch path.
//
// Footprint: 256 threads, no LDS, no atomics (k_site_compare), no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "exact_sum_kernels.hpp"
#include "nt_kernels.hpp"

namespace dynk {

// One group of G lanes over `cnt` counters of both sites, ROUNDS * G >= cnt: lane l holds the counters l, l + G, ... of BOTH
// sites, so a group's loads are neighbouring words. Two inclusive prefix sums by __shfl_up within the group, the round's total
// carried by __shfl; then the products, and the maximum of (d, index) over the group by a butterfly of 64-bit shuffles, ties to
// the smaller index. A counter index >= cnt holds 0: its prefix sums are the totals, its d is 0 and it never beats a smaller index.
template <int G, int ROUNDS>
__device__ __forceinline__ void sc_group(const unsigned int* __restrict__ ha, const unsigned int* __restrict__ hb, uint32_t cnt, bool live,
                                         int l, uint32_t& n_a, uint32_t& n_b, unsigned long long& num, uint32_t& at, int& side) {
  uint32_t pa[ROUNDS], pb[ROUNDS];
  uint32_t ca = 0, cb = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const uint32_t e = (uint32_t)(r * G + l);
    const bool in = live && e < cnt;
    uint32_t va = in ? ha[e] : 0u, vb = in ? hb[e] : 0u;
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
      const uint32_t ua = __shfl_up(va, d, G), ub = __shfl_up(vb, d, G);
      if (l >= d) {
        va += ua;
        vb += ub;
      }
    }
    pa[r] = va + ca;
    pb[r] = vb + cb;
    ca = __shfl(pa[r], G - 1, G);
    cb = __shfl(pb[r], G - 1, G);
  }
  n_a = ca;
  n_b = cb;
  unsigned long long best = 0;
  uint32_t best_e = (uint32_t)l;
  int best_s = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const unsigned long long x = (unsigned long long)pa[r] * n_b, y = (unsigned long long)pb[r] * n_a;
    const unsigned long long d = x > y ? x - y : y - x;
    if (r == 0 || d > best) {  // rounds run in rising index: a later equal d does not replace an earlier one
      best = d;
      best_e = (uint32_t)(r * G + l);
      best_s = x > y ? 1 : (x < y ? -1 : 0);
    }
  }
#pragma unroll
  for (int m = 1; m < G; m <<= 1) {
    const unsigned long long od = __shfl_xor(best, m, G);
    const uint32_t oe = __shfl_xor(best_e, m, G);
    const int os = __shfl_xor(best_s, m, G);
    if (od > best || (od == best && oe < best_e)) {
      best = od;
      best_e = oe;
      best_s = os;
    }
  }
  const bool empty = n_a == 0 || n_b == 0;
  num = empty ? 0ull : best;
  at = empty ? SC_NO_AT : best_e;
  side = empty ? 0 : best_s;
}

// A group of G = min(64, the power of two >= Bc) lanes owns one site pair: at most four rounds over the level counters
// (Bc <= 256), and the 16 dwell counters behind them by the same lanes (16 / G rounds for G = 4 and G = 8). Lanes of pairs
// outside the window load nothing and store nothing. The two windows may lie anywhere in the table, in either order, and may
// overlap: nothing is written to the table. Block of 256.
template <int G>
__global__ __launch_bounds__(256) void k_site_compare(SiteCompare sc) {
  constexpr int ROUNDS = G == 64 ? 4 : 1;
  constexpr int DROUNDS = G >= SH_DWELL_BINS ? 1 : SH_DWELL_BINS / G;
  const uint32_t B = sc.bins + 2u, H = B + (uint32_t)SH_DWELL_BINS;
  const int l = (int)(threadIdx.x & 63u) & (G - 1);
  const uint64_t pair = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / (uint32_t)G;
  const bool live = pair < sc.count;
  const unsigned int* __restrict__ ha = sc.hist_a + pair * H;
  const unsigned int* __restrict__ hb = sc.hist_b + pair * H;
  uint32_t n_a, n_b, d_na, d_nb, l_at, d_at;
  unsigned long long l_num, d_num;
  int l_side, d_side;
  sc_group<G, ROUNDS>(ha, hb, B, live, l, n_a, n_b, l_num, l_at, l_side);
  sc_group<G, DROUNDS>(ha + B, hb + B, (uint32_t)SH_DWELL_BINS, live, l, d_na, d_nb, d_num, d_at, d_side);
  if (live && l == 0) {
    const uint64_t c = sc.count;
    unsigned long long* __restrict__ o64 = sc.out;
    o64[pair] = l_num;
    o64[c + pair] = d_num;
    uint32_t* __restrict__ o32 = reinterpret_cast<uint32_t*>(o64 + 2 * c);
    o32[pair] = n_a;
    o32[c + pair] = n_b;
    o32[2 * c + pair] = l_at;
    o32[3 * c + pair] = d_at;
    o32[4 * c + pair] = (uint32_t)l_side;
    o32[5 * c + pair] = (uint32_t)d_side;
  }
}

inline void launch_site_compare_kernel(const SiteCompare& sc, hipStream_t s) {
  if (!sc.hist_a || !sc.hist_b || !sc.out || sc.count == 0 || sc.bins < 2 || sc.bins > (uint32_t)SH_BINS_MAX) return;
  const uint32_t B = sc.bins + 2u;
  uint32_t G = 4;
  while (G < B && G < 64) G <<= 1;
  const unsigned blocks = (unsigned)(((uint64_t)sc.count * G + 255u) / 256u);
  switch (G) {
    case 4: hipLaunchKernelGGL(k_site_compare<4>, dim3(blocks), dim3(256), 0, s, sc); break;
    case 8: hipLaunchKernelGGL(k_site_compare<8>, dim3(blocks), dim3(256), 0, s, sc); break;
    case 16: hipLaunchKernelGGL(k_site_compare<16>, dim3(blocks), dim3(256), 0, s, sc); break;
    case 32: hipLaunchKernelGGL(k_site_compare<32>, dim3(blocks), dim3(256), 0, s, sc); break;
    default: hipLaunchKernelGGL(k_site_compare<64>, dim3(blocks), dim3(256), 0, s, sc); break;
  }
}

// The add (dyn_aligner_site_summary_add): one window of `count` sites from a staging buffer. Thread t < count adds the seven
// staged u64 of site t into the table's cell: n_rows, n_samples, dwell_sq by 64-bit atomic adds (mod 2^64), M1 and M2 as 128-bit
// two's complement through xs_add128 (the carry of the low limb goes into the high one, mod 2^128). The threads behind them add
// the count * width staged counters with 32-bit atomicAdd (mod 2^32), when there are any. Thread 0 also adds the caller's five
// totals. The atomics are the filling kernels' own, at device scope: a ticket of a resident session that is still adding loses no
// update. A zero adds nothing and is not sent.
__global__ __launch_bounds__(256) void k_site_add(SiteAdd sa) {
  const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t words = sa.hist ? (uint64_t)sa.count * sa.width : 0ull;
  if (t < sa.count) {
    const unsigned long long* __restrict__ src = sa.cols + t * SS_FIELDS;
    unsigned long long* cell = sa.acc + t * SS_FIELDS;
#pragma unroll
    for (int f = 0; f < 3; ++f)
      if (src[f]) atomicAdd(cell + f, src[f]);
    xs_add128(cell + 3, src[3], src[4]);
    xs_add128(cell + 5, src[5], src[6]);
    if (t == 0 && sa.add_totals)
      for (int f = 0; f < SS_TOTALS; ++f)
        if (sa.totals_in[f]) atomicAdd(sa.totals + f, sa.totals_in[f]);
  } else if (t - sa.count < words) {
    const uint64_t w = t - sa.count;
    const unsigned int v = sa.counters[w];
    if (v) atomicAdd(sa.hist + w, v);
  }
}

inline void launch_site_add_kernel(const SiteAdd& sa, hipStream_t s) {
  if (!sa.acc || !sa.totals || !sa.cols || sa.count == 0 || (sa.hist && (!sa.counters || sa.width == 0))) return;
  const uint64_t threads = (uint64_t)sa.count + (sa.hist ? (uint64_t)sa.count * sa.width : 0ull);
  hipLaunchKernelGGL(k_site_add, dim3((unsigned)((threads + 255u) / 256u)), dim3(256), 0, s, sa);
}

}  // namespace dynk
