// Test unit of tests/test_gpu_soft_levels_kernels.py: soft_level_kernels.hpp (the wave sweep of the read queue and the column walk
// of the banded-lattice kernel, over the three accessor pairs of border_kernels.hpp / sample_kernels.hpp) compiled with the
// product's flags and run on a lattice the test writes itself. sl_run runs one read:
//   mode 0  separate layout, wave sweep     mode 1  in-place layout, wave sweep
//   mode 2  wide layout, wave sweep         mode 3  wide layout, one thread per column (256 threads)
// and returns per column n = 1 .. N-1, at index n - 1, the three raw sums; and the device's own term
// g = exp(LPM(t, n)) + exp(LPE(t, n)) of every in-band cell, terms[t * (2 bw + 1) + (n - start(t))], so that the host can form the
// sums of the same terms and hold every result to the bit.
// layouts as in border_interval.hip: separate (lpe [rows][P] float, bE [rows][P] double, samples, emissions, Zb, m1; lattice row
// t lives in row rowmap[t] of the arrays, as a page table would place it), in place (lp [rows][P][2] float), wide
// (lp [T][2 bw + 3][2]).
#include <cstdint>

#include <hip/hip_runtime.h>

#include "soft_level_kernels.hpp"

using namespace dynk;

namespace {

struct RowMap {
  const uint32_t* map;
  __device__ uint32_t operator()(int t) const { return map[t]; }
};

struct Job {
  int mode, T, N, bw;
  double ratio, Zb, m1;
  const uint32_t* rowmap;
  const float* lp;
  const double* bE;
  const double* sig;
  const Emis* par;
  double* sums;   // [3][N - 1]
  double* terms;  // [T][2 bw + 1]
};

template <class LPM, class LPE>
__device__ void run_cell(const LPM& lpm, const LPE& lpe, const BorderBand& band, const Job& j) {
  const int cols = j.N - 1;
  auto sink = [&](int n, const SoftColumn& c) {
    j.sums[n - 1] = c.w;
    j.sums[cols + n - 1] = c.s1;
    j.sums[2 * cols + n - 1] = c.s2;
  };
  if (j.mode == 3) {
    for (int n = 1 + (int)threadIdx.x; n < j.N; n += (int)blockDim.x) {
      SoftColumn c;
      soft_column_walk(lpm, lpe, band, j.sig, n, c);
      sink(n, c);
    }
  } else if (threadIdx.x < 64) {
    soft_sweep_wave(lpm, lpe, band, j.sig, (int)threadIdx.x, sink);
  }
}

template <class LPM, class LPE>
__device__ void terms_cell(const LPM& lpm, const LPE& lpe, const BorderBand& band, const Job& j) {
  const int W = 2 * j.bw + 1;
  for (int t = 1 + (int)blockIdx.x; t < j.T; t += (int)gridDim.x)
    for (int c = (int)threadIdx.x; c < W; c += (int)blockDim.x) {
      const int n = band.start(t) + c;
      if (band.holds(t, n)) j.terms[(size_t)t * W + c] = soft_term(lpm, lpe, t, n);
    }
}

template <bool TERMS>
__global__ __launch_bounds__(256) void k_run(const Job j) {
  const BorderBand band{j.T, j.N, j.bw, j.ratio};
  const RowMap rm{j.rowmap};
  if (j.mode == 0) {
    const BorderCellSeparate<RowMap> lpm{band, j.lp, j.bE, j.sig, j.par, j.Zb, j.m1, rm};
    const SampleLpeSeparate<RowMap> lpe{band, j.lp, rm};
    if (TERMS) terms_cell(lpm, lpe, band, j); else run_cell(lpm, lpe, band, j);
  } else if (j.mode == 1) {
    const BorderCellInplace<RowMap> lpm{band, j.lp, rm};
    const SampleLpeInplace<RowMap> lpe{band, j.lp, rm};
    if (TERMS) terms_cell(lpm, lpe, band, j); else run_cell(lpm, lpe, band, j);
  } else {
    const BorderCellWide lpm{band, j.lp};
    const SampleLpeWide lpe{band, j.lp};
    if (TERMS) terms_cell(lpm, lpe, band, j); else run_cell(lpm, lpe, band, j);
  }
}

}  // namespace

#define TRY(x)                      \
  do {                              \
    err[k++] = (int)(x);            \
    if (err[k - 1]) return k;       \
  } while (0)

// every pointer is host memory; sums [3][N - 1] and terms [T][2 bw + 1] are filled by the caller (the fill stays where nothing is
// written); returns the number of steps taken, err[step] = hipError_t of each. The array sizes are checked against what the
// sweeps may address: rowmap T + 1 entries below `rows`, lp / bE `rows` stored rows (wide: T rows of 2 bw + 3), sig T - 1, par N - 1.
extern "C" int sl_run(int mode, int T, int N, int bw, double ratio, double Zb, double m1, uint64_t n_rowmap, const uint32_t* rowmap,
                      uint64_t n_lp, const float* lp, uint64_t n_bE, const double* bE, uint64_t n_sig, const double* sig,
                      uint64_t n_par, const double* par4, double* sums, double* terms, int* err) {
  int k = 0;
  bool ok = mode >= 0 && mode <= 3 && N >= 2 && T >= 3 && bw >= 1 && 2 * bw + 1 <= P - 1 && n_sig == (uint64_t)T - 1 &&
            n_par == (uint64_t)N - 1 && n_rowmap == (uint64_t)T + 1;
  if (ok) {
    uint64_t rows = 0;
    for (uint64_t i = 0; i < n_rowmap; ++i) rows = rowmap[i] + 1 > rows ? rowmap[i] + 1 : rows;
    if (mode == 0) ok = n_lp >= rows * P && n_bE >= rows * P;
    else if (mode == 1) ok = n_lp >= rows * P * 2;
    else ok = n_lp >= (uint64_t)T * (2 * (uint64_t)bw + 3) * 2;
  }
  if (!ok) {
    err[k++] = (int)hipErrorInvalidValue;
    return k;
  }
  const uint64_t cols = (uint64_t)N - 1, n_terms = (uint64_t)T * (2 * (uint64_t)bw + 1);
  uint32_t* d_map = nullptr;
  float* d_lp = nullptr;
  double *d_bE = nullptr, *d_sig = nullptr, *d_par = nullptr, *d_sums = nullptr, *d_terms = nullptr;
  auto up = [&](auto** d, const void* h, uint64_t bytes) -> hipError_t {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), bytes ? bytes : 8);
    if (e == hipSuccess && bytes) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
    return e;
  };
  TRY(up(&d_map, rowmap, n_rowmap * 4));
  TRY(up(&d_lp, lp, n_lp * 4));
  TRY(up(&d_bE, bE, n_bE * 8));
  TRY(up(&d_sig, sig, n_sig * 8));
  TRY(up(&d_par, par4, n_par * sizeof(Emis)));
  static_assert(sizeof(Emis) == 32, "mean, inv_stdev, neg_log_stdev, stdev");
  TRY(up(&d_sums, sums, 3 * cols * 8));
  TRY(up(&d_terms, terms, n_terms * 8));
  Job j{};
  j.mode = mode;
  j.T = T;
  j.N = N;
  j.bw = bw;
  j.ratio = ratio;
  j.Zb = Zb;
  j.m1 = m1;
  j.rowmap = d_map;
  j.lp = d_lp;
  j.bE = d_bE;
  j.sig = d_sig;
  j.par = reinterpret_cast<const Emis*>(d_par);
  j.sums = d_sums;
  j.terms = d_terms;
  hipLaunchKernelGGL(k_run<false>, dim3(1), dim3(mode == 3 ? 256 : 64), 0, 0, j);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_run<true>, dim3(64), dim3(64), 0, 0, j);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(sums, d_sums, 3 * cols * 8, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(terms, d_terms, n_terms * 8, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_map, (void*)d_lp, (void*)d_bE, (void*)d_sig, (void*)d_par, (void*)d_sums, (void*)d_terms}) (void)hipFree(p);
  return k;
}
