// Test unit of tests/test_gpu_border_interval.py: interval_kernels.hpp (the wave sweep of the read queue and the column walk of
// the banded-lattice kernel, over border_kernels.hpp's three cell accessors) compiled with the product's flags and run on a
// lattice the test writes itself. bi_run runs one read:
//   mode 0  separate layout, wave sweep     mode 1  in-place layout, wave sweep
//   mode 2  wide layout, wave sweep         mode 3  wide layout, one thread per column (256 threads)
// and returns per column n = 1 .. N-1, at index n - 1: lo and hi (positions, as the product stores them) and the raw S, A, B; and
// the device's own term exp(LPM(t, n)) of every in-band cell, terms[t * (2 bw + 1) + (n - start(t))], so that the host can form
// the sums of the same terms and hold every result to the bit.
// layouts as in posterior_samples.hip: separate (lpe [rows][P] float, bE [rows][P] double, samples, emissions, Zb, m1; lattice
// row t lives in row rowmap[t] of the arrays, as a page table would place it), in place (lp [rows][P][2] float), wide
// (lp [T][2 bw + 3][2]).
#include <cstdint>

#include <hip/hip_runtime.h>

#include "interval_kernels.hpp"

using namespace dynk;

namespace {

struct RowMap {
  const uint32_t* map;
  __device__ uint32_t operator()(int t) const { return map[t]; }
};

struct Job {
  int mode, T, N, bw;
  double ratio, Zb, m1, tail;
  const uint32_t* rowmap;
  const float* lp;
  const double* bE;
  const double* sig;
  const Emis* par;
  const uint32_t* rows;  // [N - 1] r of every column
  uint32_t* lo;          // [N - 1] each
  uint32_t* hi;
  double* sab;           // [3][N - 1]
  double* terms;         // [T][2 bw + 1]
};

template <class CELL>
__device__ void run_cell(const CELL& cell, const BorderBand& band, const Job& j) {
  const int cols = j.N - 1;
  auto sink = [&](int n, const IntervalColumn& c, int) {
    j.lo[n - 1] = c.lo_pos();
    j.hi[n - 1] = c.hi_pos();
    j.sab[n - 1] = c.C;
    j.sab[cols + n - 1] = c.A;
    j.sab[2 * cols + n - 1] = c.B;
  };
  if (j.mode == 3) {
    for (int n = 1 + (int)threadIdx.x; n < j.N; n += (int)blockDim.x) {
      IntervalColumn c;
      interval_column_walk(cell, band, n, (int)j.rows[n - 1], j.tail, c);
      sink(n, c, 0);
    }
  } else if (threadIdx.x < 64) {
    interval_sweep_wave(cell, band, j.rows, j.tail, (int)threadIdx.x, sink);
  }
}

template <class CELL>
__device__ void terms_cell(const CELL& cell, const BorderBand& band, const Job& j) {
  const int W = 2 * j.bw + 1;
  for (int t = 1 + (int)blockIdx.x; t < j.T; t += (int)gridDim.x)
    for (int c = (int)threadIdx.x; c < W; c += (int)blockDim.x) {
      const int n = band.start(t) + c;
      if (band.holds(t, n)) j.terms[(size_t)t * W + c] = border_term(cell, t, n);
    }
}

template <bool TERMS>
__global__ __launch_bounds__(256) void k_run(const Job j) {
  const BorderBand band{j.T, j.N, j.bw, j.ratio};
  const RowMap rm{j.rowmap};
  if (j.mode == 0) {
    const BorderCellSeparate<RowMap> cell{band, j.lp, j.bE, j.sig, j.par, j.Zb, j.m1, rm};
    if (TERMS) terms_cell(cell, band, j); else run_cell(cell, band, j);
  } else if (j.mode == 1) {
    const BorderCellInplace<RowMap> cell{band, j.lp, rm};
    if (TERMS) terms_cell(cell, band, j); else run_cell(cell, band, j);
  } else {
    const BorderCellWide cell{band, j.lp};
    if (TERMS) terms_cell(cell, band, j); else run_cell(cell, band, j);
  }
}

}  // namespace

#define TRY(x)                      \
  do {                              \
    err[k++] = (int)(x);            \
    if (err[k - 1]) return k;       \
  } while (0)

// every pointer is host memory; lo, hi [N - 1], sab [3][N - 1] and terms [T][2 bw + 1] are filled by the caller (the fill stays
// where nothing is written); returns the number of steps taken, err[step] = hipError_t of each
extern "C" int bi_run(int mode, int T, int N, int bw, double ratio, double Zb, double m1, double tail, uint64_t n_rowmap,
                      const uint32_t* rowmap, uint64_t n_lp, const float* lp, uint64_t n_bE, const double* bE, uint64_t n_sig,
                      const double* sig, uint64_t n_par, const double* par4, const uint32_t* rows, uint32_t* lo, uint32_t* hi,
                      double* sab, double* terms, int* err) {
  int k = 0;
  if (mode < 0 || mode > 3 || N < 2 || T < 3 || bw < 1 || 2 * bw + 1 > P - 1 || !(tail > 0.0 && tail < 0.5)) {
    err[k++] = (int)hipErrorInvalidValue;
    return k;
  }
  const uint64_t cols = (uint64_t)N - 1, n_terms = (uint64_t)T * (2 * (uint64_t)bw + 1);
  uint32_t *d_map = nullptr, *d_rows = nullptr, *d_lo = nullptr, *d_hi = nullptr;
  float* d_lp = nullptr;
  double *d_bE = nullptr, *d_sig = nullptr, *d_par = nullptr, *d_sab = nullptr, *d_terms = nullptr;
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
  TRY(up(&d_rows, rows, cols * 4));
  TRY(up(&d_lo, lo, cols * 4));
  TRY(up(&d_hi, hi, cols * 4));
  TRY(up(&d_sab, sab, 3 * cols * 8));
  TRY(up(&d_terms, terms, n_terms * 8));
  Job j{};
  j.mode = mode;
  j.T = T;
  j.N = N;
  j.bw = bw;
  j.ratio = ratio;
  j.Zb = Zb;
  j.m1 = m1;
  j.tail = tail;
  j.rowmap = d_map;
  j.lp = d_lp;
  j.bE = d_bE;
  j.sig = d_sig;
  j.par = reinterpret_cast<const Emis*>(d_par);
  j.rows = d_rows;
  j.lo = d_lo;
  j.hi = d_hi;
  j.sab = d_sab;
  j.terms = d_terms;
  hipLaunchKernelGGL(k_run<false>, dim3(1), dim3(mode == 3 ? 256 : 64), 0, 0, j);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  hipLaunchKernelGGL(k_run<true>, dim3(64), dim3(64), 0, 0, j);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(lo, d_lo, cols * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(hi, d_hi, cols * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(sab, d_sab, 3 * cols * 8, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(terms, d_terms, n_terms * 8, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_map, (void*)d_lp, (void*)d_bE, (void*)d_sig, (void*)d_par, (void*)d_rows, (void*)d_lo, (void*)d_hi,
                  (void*)d_sab, (void*)d_terms})
    (void)hipFree(p);
  return k;
}
