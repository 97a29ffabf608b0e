// lpe_liveness.hip -- test-only translation unit (tests/test_gpu_lpe_liveness.py): the forward sweep's liveness helpers
// (lpe_liveness.hpp: lpe_lane_live, lpe_store_mask) run on rows of floats the HOST hands in, one wave per row, with the
// row's cells dealt to the lanes as the sweep holds them (lane l owns band slots 7 l .. 7 l + 6). Both masks of every row
// are compared with a three-line NumPy restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lpe_liveness.hpp"

namespace {

// grid = rows, block = one wave; out[2 r] = live lanes, out[2 r + 1] = store-live lanes (whole groups)
__global__ __launch_bounds__(64) void k_liveness(const float* __restrict__ rows, int n_rows, float floor, uint64_t* __restrict__ out) {
  const int r = blockIdx.x, lane = threadIdx.x;
  if (r >= n_rows) return;
  float f[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) f[j] = rows[(size_t)r * 448 + lane * 7 + j];
  const bool live = dynk::lpe_lane_live(f, floor);
  const uint64_t lanes = __ballot(live);
  const uint64_t groups = dynk::lpe_store_mask(live);
  if (lane == 0) {
    out[2 * (size_t)r] = lanes;
    out[2 * (size_t)r + 1] = groups;
  }
}

}  // namespace

// rows[n_rows][448] floats (bit patterns as handed in), out[2 * n_rows]. Every HIP call's hipError_t goes into err[] in order
// (at most 16); returns how many were made, or -1 for a bad argument. The first failing step ends the run.
extern "C" int lv_run(int n_rows, const float* rows, float floor, uint64_t* out, int* err) {
  if (n_rows < 1 || n_rows > 65535 || !rows || !out || !err) return -1;
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
  };
  void *d_rows = nullptr, *d_out = nullptr;
  const size_t b_rows = (size_t)n_rows * 448 * 4, b_out = (size_t)n_rows * 16;
  step(hipMalloc(&d_rows, b_rows));
  if (ok) step(hipMalloc(&d_out, b_out));
  if (ok) step(hipMemcpy(d_rows, rows, b_rows, hipMemcpyHostToDevice));
  if (ok) step(hipMemset(d_out, 0xff, b_out));
  if (ok) {
    hipLaunchKernelGGL(k_liveness, dim3(n_rows), dim3(64), 0, 0, static_cast<const float*>(d_rows), n_rows, floor,
                       static_cast<uint64_t*>(d_out));
    step(hipGetLastError());
  }
  if (ok) step(hipDeviceSynchronize());
  if (ok) step(hipMemcpy(out, d_out, b_out, hipMemcpyDeviceToHost));
  for (void* p : {d_out, d_rows})
    if (p) step(hipFree(p));
  return k;
}
