// sample_kernels.hpp -- posterior path sampling (dyn_aligner_set_posterior_samples): K complete alignments of a read drawn from
// the lattice's posterior distribution over paths, each returned as its segment starts. Included by nt_kernels.hip and
// band_reads.hip (the phase behind traceback / mpost and behind the border-confidence phase, while the read's lattice is still
// in its pages or arena) and by tests/device_math/posterior_samples.hip, which runs the walk on a lattice the test writes itself.
//
// Definition (include/dynamont_mi.h). LPM(t, n) / LPE(t, n): the log-posteriors of the M and the E cell
// of lattice row t = 0 .. T-1 and column n = 0 .. N-1, -inf outside the reference's band window of the row, LPM -inf in row 0,
// LPE(0, 0) = 0 -- the values the border-confidence accessors (border_kernels.hpp) define.
//   u(seed, i, k, t) = (mix(mix(mix(seed + i) + k) + t) >> 11) * 2^-53, mix = the SplitMix64 step, i = the read's index in its
//   batch or ticket, k = the sample, t = the row of the cell at which the choice is made.
// Sample k of read i starts in E(0, 0). While (t, n) != (T-1, N-1): a = LPM(t+1, n+1) (-inf when n+1 >= N or t+1 > T-1),
// b = LPE(t+1, n). Both -inf: the sample is dead. One finite: that way, no number drawn. Both finite: p = exp(a - LPE(t, n)) in
// fp64, move iff u(seed, i, k, t) < p. A move records sample_start[k][n] = t and continues in E(t+2, n+1) (an M cell has one
// way on), a stay continues in E(t+1, n). M(t+1, n+1) has the single predecessor E(t, n), so P(move | E(t, n)) is that
// quotient: the walk samples the posterior exactly. Every step advances t: at most T steps.
// A dead sample has all its entries 0xFFFFFFFF and is counted in sample_dead[i].
// A cell accessor is "the log-posterior or -inf"; each LPM accessor of border_kernels.hpp gets its LPE twin here:
//   SampleLpeSeparate  separate layout (JOB_ALIGN): the float LPE of the cell
//   SampleLpeInplace   in-place layout (JOB_ALIGN_INPLACE): the float LPE half of the slot
//   SampleLpeWide      band_reads.hip (diagonal window): lp[2 * cell + 1]
// with the same explicit band checks and clamped addresses (a band slot outside the band carries anything).
// Lane mapping: one lane per sample (k < K <= 64); the lanes of the wave walk side by side, each at its own cell. Output is
// sample-major, uint32 [K][capacity] at k * capacity + seg_off + j: a lane writes ascending addresses of its own plane. No wait,
// no atomic, no LDS, no scratch memory; the result depends on the read's lattice, its index and the seed alone.
#pragma once

#include "border_kernels.hpp"

namespace dynk {

constexpr int PS_MAX_SAMPLES = 64;            // = DYN_POSTERIOR_SAMPLES_MAX: one wave
constexpr uint32_t PS_DEAD = 0xFFFFFFFFu;     // every entry of a dead sample

__device__ __forceinline__ uint64_t sample_mix(uint64_t x) {  // the SplitMix64 step
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// key = mix(mix(seed + i) + k): the part of u that does not depend on the row
__device__ __forceinline__ double sample_uniform(uint64_t key, int t) {
  return (double)(sample_mix(key + (uint64_t)t) >> 11) * 0x1p-53;
}

// E(0, 0) is the one cell of row 0 (LPE = 0: every path starts there); column 0 holds nothing else (BorderBand::holds)
template <class ROW>
struct SampleLpeSeparate {
  BorderBand band;
  const float* __restrict__ lpe;  // [row][P] float LPE
  ROW row;
  __device__ __forceinline__ double operator()(int t, int n) const {
    const float l = lpe[(size_t)row(border_clamp(t, 0, band.T)) * P + border_row_pos(n % P)];
    return (t == 0 && n == 0) ? 0.0 : band.holds(t, n) ? (double)l : dynmath::NEG_INF;
  }
};

template <class ROW>
struct SampleLpeInplace {
  BorderBand band;
  const float* __restrict__ lp;  // [row][P] (float LPM, float LPE)
  ROW row;
  __device__ __forceinline__ double operator()(int t, int n) const {
    const float l = lp[2 * ((size_t)row(border_clamp(t, 0, band.T)) * P + border_row_pos(n % P)) + 1];
    return (t == 0 && n == 0) ? 0.0 : band.holds(t, n) ? (double)l : dynmath::NEG_INF;
  }
};

struct SampleLpeWide {
  BorderBand band;
  const float* __restrict__ lp;  // [t][2 bw + 3] (float LPM, float LPE), band column c = n - start_t + 1
  __device__ __forceinline__ double operator()(int t, int n) const {
    const int tc = border_clamp(t, 0, band.T - 1), B = 2 * band.bw + 3;
    const int c = border_clamp(n - band.start(tc) + 1, 0, B - 1);
    const float l = lp[2 * ((size_t)tc * (size_t)B + c) + 1];
    return (t == 0 && n == 0) ? 0.0 : band.holds(t, n) ? (double)l : dynmath::NEG_INF;
  }
};

// one sample: the walk of lane k through the read's lattice; returns whether it died. `out` is the sample's own row of the
// read, N - 1 entries. The accessors are only called for cells whose every address lies inside the read's lattice: rows are
// clamped by them, and the M column is held below N here (a term that does not exist is decided from t and n alone).
template <class LPM, class LPE>
__device__ __forceinline__ bool posterior_sample_walk(const LPM& cell_lpm, const LPE& cell_lpe, int T, int N, uint64_t key,
                                                      uint32_t* __restrict__ out) {
  int t = 0, n = 0;
  double here = 0.0;  // LPE(t, n)
  bool dead = false;
#pragma unroll 1
  while (t != T - 1 || n != N - 1) {
    if (t >= T - 1) {  // the last row off the corner: neither way exists
      dead = true;
      break;
    }
    const bool col = n + 1 < N;
    const double am = cell_lpm(t + 1, col ? n + 1 : N - 1);
    const double a = col ? am : dynmath::NEG_INF;
    const double b = cell_lpe(t + 1, n);
    const bool fa = a != dynmath::NEG_INF, fb = b != dynmath::NEG_INF;
    if (!fa && !fb) {
      dead = true;
      break;
    }
    bool move = fa;
    if (fa && fb) move = sample_uniform(key, t) < exp(a - here);
    if (move) {
      out[n] = (uint32_t)t;
      here = cell_lpe(t + 2, n + 1);
      t += 2;
      n += 1;
    } else {
      here = b;
      t += 1;
    }
  }
  if (dead)
    for (int j = 0; j < N - 1; ++j) out[j] = PS_DEAD;
  return dead;
}

// the phase: called by ONE WHOLE WAVE (lane = 0 .. 63); lane k < K walks sample k, the others wait for the count
template <class LPM, class LPE>
__device__ __forceinline__ void posterior_samples_read(const LPM& cell_lpm, const LPE& cell_lpe, const ReadDesc& rd,
                                                       const SampleOut& so, int lane) {
  const int T = (int)rd.T, N = (int)rd.N;
  bool dead = false;
  if (lane < so.count && N >= 2) {
    const uint64_t key = sample_mix(sample_mix(so.seed + (uint64_t)rd.read) + (uint64_t)lane);
    dead = posterior_sample_walk(cell_lpm, cell_lpe, T, N, key, so.start + (size_t)lane * so.capacity + rd.seg_off);
  }
  const uint64_t died = __ballot(dead);
  if (lane == 0) so.start[(size_t)so.count * so.capacity + rd.read] = (uint32_t)__popcll(died);  // the dead counts: behind the planes
}

}  // namespace dynk
