// site_quantile_kernels.hpp -- quantiles of a window of the per-site level histograms (dyn_aligner_site_quantiles), reduced on
// the device: the histograms (site_summary_kernels.hpp fills them) stay where they are, a few words per site come back. Included
// by site_summary.hip (launch_site_quantiles) and by tests/device_math/site_histogram.hip, which runs the kernel on histograms
// the test uploads and compares every output integer with a Python-int restatement (tests/test_gpu_site_histogram.py).
// Footprint: 256 threads, no LDS, no atomics, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "nt_kernels.hpp"

namespace dynk {

// Quantiles of the level histograms of the sites [0, sq.count) behind sq.hist. B = bins + 2 counters per site; a group of
// G = min(64, the power of two >= B) lanes owns a site, lane l of it the counters l, l + G, l + 2 G, l + 3 G (B <= 256: at most
// four), so the lanes of a group load neighbouring words. Per counter the inclusive prefix sum over the site (uint32: n < 2^32
// is the defined domain); per probability q: n = the total, k = min(max(ceil(q n), 1), n), bin = the first counter whose prefix
// reaches k (a ballot over the group, round by round), below = the prefix in front of it, in_bin = its count. n = 0: bin =
// SQ_NO_BIN, rank = below = in_bin = 0. Lanes whose site lies outside the window load nothing and store nothing. Block of 256.
template <int G>
__global__ __launch_bounds__(256) void k_site_quantiles(SiteQuantiles sq) {
  constexpr int ROUNDS = G == 64 ? 4 : 1;
  const uint32_t B = sq.bins + 2u, H = B + (uint32_t)SH_DWELL_BINS;
  const int lane = (int)(threadIdx.x & 63u), l = lane & (G - 1), g0 = lane & ~(G - 1);
  const uint64_t site = ((uint64_t)blockIdx.x * 256u + threadIdx.x) / (uint32_t)G;
  const bool live = site < sq.count;
  const unsigned int* __restrict__ h = sq.hist + site * H;
  uint32_t c[ROUNDS], p[ROUNDS];
  uint32_t carry = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const uint32_t e = (uint32_t)(r * G + l);
    c[r] = (live && e < B) ? h[e] : 0u;
    uint32_t v = c[r];
#pragma unroll
    for (int d = 1; d < G; d <<= 1) {
      const uint32_t up = __shfl_up(v, d, G);
      if (l >= d) v += up;
    }
    p[r] = v + carry;
    carry = __shfl(p[r], G - 1, G);
  }
  const uint32_t n = carry;
  const uint64_t gmask = G == 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
  uint32_t* __restrict__ out = sq.out;
  if (live && l == 0) out[site] = n;
  for (int q = 0; q < sq.n_probs; ++q) {
    uint32_t k = (uint32_t)ceil(__dmul_rn(sq.probs[q], (double)n));
    k = min(max(k, 1u), n);
    uint32_t bin = SQ_NO_BIN, below = 0, in_bin = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const uint64_t hit = (__ballot(n != 0 && p[r] >= k) >> g0) & gmask;
      const int src = hit ? __ffsll((unsigned long long)hit) - 1 : 0;
      const uint32_t pb = __shfl(p[r], src, G), cb = __shfl(c[r], src, G);
      if (hit && bin == SQ_NO_BIN) {
        bin = (uint32_t)(r * G + src);
        in_bin = cb;
        below = pb - cb;
      }
    }
    if (live && l == 0) {
      const uint64_t o = site * (uint32_t)sq.n_probs + (uint32_t)q;
      const uint64_t col = (uint64_t)sq.count * (uint32_t)sq.n_probs;  // one [count][n_probs] array
      uint32_t* __restrict__ base = out + sq.count;
      base[o] = n ? k : 0u;
      base[col + o] = bin;
      base[2 * col + o] = below;
      base[3 * col + o] = in_bin;
    }
  }
}

inline void launch_site_quantiles_kernel(const SiteQuantiles& sq, hipStream_t s) {
  if (!sq.hist || !sq.out || sq.count == 0 || sq.n_probs < 1 || sq.n_probs > SQ_PROBS_MAX || sq.bins < 2 || sq.bins > (uint32_t)SH_BINS_MAX) return;
  const uint32_t B = sq.bins + 2u;
  uint32_t G = 4;
  while (G < B && G < 64) G <<= 1;
  const unsigned blocks = (unsigned)(((uint64_t)sq.count * G + 255u) / 256u);
  switch (G) {
    case 4: hipLaunchKernelGGL(k_site_quantiles<4>, dim3(blocks), dim3(256), 0, s, sq); break;
    case 8: hipLaunchKernelGGL(k_site_quantiles<8>, dim3(blocks), dim3(256), 0, s, sq); break;
    case 16: hipLaunchKernelGGL(k_site_quantiles<16>, dim3(blocks), dim3(256), 0, s, sq); break;
    case 32: hipLaunchKernelGGL(k_site_quantiles<32>, dim3(blocks), dim3(256), 0, s, sq); break;
    default: hipLaunchKernelGGL(k_site_quantiles<64>, dim3(blocks), dim3(256), 0, s, sq); break;
  }
}

}  // namespace dynk
