// Test unit of tests/test_gpu_posterior_samples.py: sample_kernels.hpp (the LPE accessors of all three lattice layouts beside
// border_kernels.hpp's LPM accessors, the walk, the dead count) compiled with the product's flags and run on a lattice the test
// writes itself. ps_run runs posterior_samples_read for one read with one wave, as the product's kernels call it:
//   out[k][seg_off + j]   sample k's start of output row j (the caller's fill stays everywhere else)
//   dead[read]            the read's dead samples (on the device they follow the K planes, as in the product)
// layout 0: separate (lpe [rows][P] float, bE [rows][P] double, samples, emissions, Zb, m1; lattice row t lives in row
// rowmap[t] of the arrays, as a page table would place it), 1: in place (lp [rows][P][2] float), 2: wide (lp [T][2 bw + 3][2]).
#include <cstdint>

#include <hip/hip_runtime.h>

#include "sample_kernels.hpp"

using namespace dynk;

namespace {

struct RowMap {
  const uint32_t* map;
  __device__ uint32_t operator()(int t) const { return map[t]; }
};

struct Job {
  int layout, bw;
  double Zb, m1;
  ReadDesc rd;
  SampleOut so;
  const uint32_t* rowmap;
  const float* lp;
  const double* bE;
  const double* sig;
  const Emis* par;
};

__global__ void k_run(const Job j) {
  const BorderBand band{(int)j.rd.T, (int)j.rd.N, j.bw, j.rd.ratio};
  const RowMap rm{j.rowmap};
  const int lane = (int)threadIdx.x;
  if (j.layout == 0)
    posterior_samples_read(BorderCellSeparate<RowMap>{band, j.lp, j.bE, j.sig, j.par, j.Zb, j.m1, rm}, SampleLpeSeparate<RowMap>{band, j.lp, rm},
                           j.rd, j.so, lane);
  else if (j.layout == 1)
    posterior_samples_read(BorderCellInplace<RowMap>{band, j.lp, rm}, SampleLpeInplace<RowMap>{band, j.lp, rm}, j.rd, j.so, lane);
  else
    posterior_samples_read(BorderCellWide{band, j.lp}, SampleLpeWide{band, j.lp}, j.rd, j.so, lane);
}

}  // namespace

#define TRY(x)                      \
  do {                              \
    err[k++] = (int)(x);            \
    if (err[k - 1]) return k;       \
  } while (0)

// every pointer is host memory; out is [K][capacity] and dead [8], both filled by the caller; returns the number of steps taken,
// err[step] = hipError_t of each
extern "C" int ps_run(int layout, int T, int N, int bw, double ratio, double Zb, double m1, int K, uint64_t seed, uint32_t read,
                      uint64_t capacity, uint64_t seg_off, uint64_t n_rowmap, const uint32_t* rowmap, uint64_t n_lp, const float* lp,
                      uint64_t n_bE, const double* bE, uint64_t n_sig, const double* sig, uint64_t n_par, const double* par4,
                      uint32_t* out, uint32_t* dead, int* err) {
  int k = 0;
  if (K < 1 || K > PS_MAX_SAMPLES || read >= 8 || seg_off + (uint64_t)N - 1 > capacity) {
    err[k++] = (int)hipErrorInvalidValue;
    return k;
  }
  uint32_t *d_map = nullptr, *d_out = nullptr;
  float* d_lp = nullptr;
  double *d_bE = nullptr, *d_sig = nullptr, *d_par = nullptr;
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
  TRY(hipMalloc(reinterpret_cast<void**>(&d_out), ((uint64_t)K * capacity + 8) * 4));
  TRY(hipMemcpy(d_out, out, (uint64_t)K * capacity * 4, hipMemcpyHostToDevice));  // the caller's fill
  TRY(hipMemcpy(d_out + (uint64_t)K * capacity, dead, 8 * 4, hipMemcpyHostToDevice));
  Job j{};
  j.layout = layout;
  j.bw = bw;
  j.Zb = Zb;
  j.m1 = m1;
  j.rd.seg_off = seg_off;
  j.rd.T = (uint32_t)T;
  j.rd.N = (uint32_t)N;
  j.rd.bw = (uint32_t)bw;
  j.rd.read = read;
  j.rd.ratio = ratio;
  j.so.start = d_out;
  j.so.capacity = capacity;
  j.so.seed = seed;
  j.so.count = K;
  j.rowmap = d_map;
  j.lp = d_lp;
  j.bE = d_bE;
  j.sig = d_sig;
  j.par = reinterpret_cast<const Emis*>(d_par);
  hipLaunchKernelGGL(k_run, dim3(1), dim3(64), 0, 0, j);
  TRY(hipGetLastError());
  TRY(hipDeviceSynchronize());
  TRY(hipMemcpy(out, d_out, (uint64_t)K * capacity * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(dead, d_out + (uint64_t)K * capacity, 8 * 4, hipMemcpyDeviceToHost));
  for (void* p : {(void*)d_map, (void*)d_lp, (void*)d_bE, (void*)d_sig, (void*)d_par, (void*)d_out}) (void)hipFree(p);
  return k;
}
