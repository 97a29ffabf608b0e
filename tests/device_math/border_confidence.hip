// Test unit of tests/test_gpu_border_confidence.py: border_kernels.hpp (the cell accessors of all three lattice layouts,
// border_term, border_window_sum) compiled with the product's flags and run on lattices the test writes itself.
// bc_run evaluates, for every border (column cols[i], M row rows[i]):
//   lpm[i][k], term[i][k]   the accessor's value and its mass at row rows[i] - W + k, k = 0 .. 2 W (rows outside 1 .. T-1: untouched)
//   here[i], sum[i]         border_window_sum's two results
// layout 0: separate (lpe [rows][P] float, bE [rows][P] double, samples, emissions, Zb, m1; lattice row t lives in row
// rowmap[t] of the arrays, as a page table would place it), 1: in place (lp [rows][P][2] float), 2: wide (lp [T][2 bw + 3][2]).
#include <cstdint>

#include <hip/hip_runtime.h>

#include "border_kernels.hpp"

using namespace dynk;

namespace {

struct RowMap {
  const uint32_t* map;
  __device__ uint32_t operator()(int t) const { return map[t]; }
};

struct Job {
  int layout, T, N, bw, W, n_borders;
  double ratio, Zb, m1;
  const int* cols;
  const int* rows;
  const uint32_t* rowmap;
  const float* lp;
  const double* bE;
  const double* sig;
  const Emis* par;
  double* lpm;
  double* term;
  double* here;
  double* sum;
};

template <class CELL>
__device__ void run(const CELL& cell, const Job& j) {
  const int K = 2 * j.W + 1;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < j.n_borders; i += gridDim.x * blockDim.x) {
    const int n = j.cols[i], r = j.rows[i];
    for (int k = 0; k < K; ++k) {
      const int t = r - j.W + k;
      if (t < 1 || t > j.T - 1) continue;
      j.lpm[(size_t)i * K + k] = cell(t, n);
      j.term[(size_t)i * K + k] = border_term(cell, t, n);
    }
    double here, sum;
    border_window_sum(cell, n, r, j.T, j.W, here, sum);
    j.here[i] = here;
    j.sum[i] = sum;
  }
}

__global__ void k_run(const Job j) {
  const BorderBand band{j.T, j.N, j.bw, j.ratio};
  const RowMap rm{j.rowmap};
  if (j.layout == 0) run(BorderCellSeparate<RowMap>{band, j.lp, j.bE, j.sig, j.par, j.Zb, j.m1, rm}, j);
  else if (j.layout == 1) run(BorderCellInplace<RowMap>{band, j.lp, rm}, j);
  else run(BorderCellWide{band, j.lp}, j);
}

}  // namespace

#define TRY(x)                      \
  do {                              \
    err[k++] = (int)(x);            \
    if (err[k - 1]) return k;       \
  } while (0)

// every pointer is host memory; returns the number of steps taken, err[step] = hipError_t of each
extern "C" int bc_run(int layout, int T, int N, int bw, int W, double ratio, double Zb, double m1, int n_borders, const int* cols,
                      const int* rows, uint64_t n_rowmap, const uint32_t* rowmap, uint64_t n_lp, const float* lp, uint64_t n_bE,
                      const double* bE, uint64_t n_sig, const double* sig, uint64_t n_par, const double* par4, double* lpm,
                      double* term, double* here, double* sum, int* err) {
  int k = 0;
  const uint64_t K = 2 * (uint64_t)W + 1;
  int *d_cols = nullptr, *d_rows = nullptr;
  uint32_t* d_map = nullptr;
  float* d_lp = nullptr;
  double *d_bE = nullptr, *d_sig = nullptr, *d_par = nullptr, *d_out = nullptr;
  auto up = [&](auto** d, const void* h, uint64_t bytes) -> hipError_t {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), bytes ? bytes : 8);
    if (e == hipSuccess && bytes) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
    return e;
  };
  TRY(up(&d_cols, cols, (uint64_t)n_borders * 4));
  TRY(up(&d_rows, rows, (uint64_t)n_borders * 4));
  TRY(up(&d_map, rowmap, n_rowmap * 4));
  TRY(up(&d_lp, lp, n_lp * 4));
  TRY(up(&d_bE, bE, n_bE * 8));
  TRY(up(&d_sig, sig, n_sig * 8));
  TRY(up(&d_par, par4, n_par * sizeof(Emis)));
  static_assert(sizeof(Emis) == 32, "mean, inv_stdev, neg_log_stdev, stdev");
  const uint64_t n_out = (uint64_t)n_borders * (2 * K + 2);
  TRY(hipMalloc(reinterpret_cast<void**>(&d_out), n_out * 8));
  TRY(hipMemcpy(d_out, lpm, (uint64_t)n_borders * K * 8, hipMemcpyHostToDevice));  // the caller's fill
  TRY(hipMemcpy(d_out + (uint64_t)n_borders * K, term, (uint64_t)n_borders * K * 8, hipMemcpyHostToDevice));
  Job j{layout, T, N, bw, W, n_borders, ratio, Zb, m1, d_cols, d_rows, d_map, d_lp, d_bE, d_sig, reinterpret_cast<const Emis*>(d_par),
        d_out, d_out + (uint64_t)n_borders * K, d_out + 2 * (uint64_t)n_borders * K, d_out + 2 * (uint64_t)n_borders * K + n_borders};
  hipLaunchKernelGGL(k_run, dim3((n_borders + 63) / 64), dim3(64), 0, 0, j);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(lpm, j.lpm, (uint64_t)n_borders * K * 8, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(term, j.term, (uint64_t)n_borders * K * 8, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(here, j.here, (uint64_t)n_borders * 8, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(sum, j.sum, (uint64_t)n_borders * 8, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_cols, (void*)d_rows, (void*)d_map, (void*)d_lp, (void*)d_bE, (void*)d_sig, (void*)d_par, (void*)d_out}) (void)hipFree(p);
  return k;
}
