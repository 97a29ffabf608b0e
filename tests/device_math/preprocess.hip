// preprocess.hip -- test-only translation unit (tests/test_gpu_preprocess_kernels.py): the product's preprocessing kernels
// (preprocess_kernels.hpp: k_normalise, k_hampel, launched by launch_preprocess exactly as the synchronous and the
// asynchronous engine launch them) run on arrays the HOST hands in. Through the product a batch reaches them only together
// with a sequence per read and lattice buffers for every sample; here a launch of 65 541 reads is a few hundred kilobytes,
// every one of the eight instantiations can be named, and every output sample is compared with the NumPy restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "preprocess_kernels.hpp"

// raw: offs[n_reads] samples of raw_dtype (0 float32, 1 int16, 2 float64, 3 int16 + calibration); read r is
// [offs[r], offs[r+1]), offs ascending (offs[0] may be > 0: samples in front of it belong to no read). shift, scale
// [n_reads]; cal_offset, cal_scale [n_reads] with raw_dtype 3, else null. out [n_out], n_out >= offs[n_reads]: filled with
// the byte `poison` on the device before the launch and copied back after it (what no read covers must still hold it).
// Every HIP call's hipError_t goes into err[] in order (at most 32); returns how many were made, or -1 for a bad argument.
// The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int pp_run(const void* raw, int raw_dtype, int compute_f32, int n_reads, const uint64_t* offs, const double* shift,
                      const double* scale, const float* cal_offset, const float* cal_scale, int W, double n_sigmas, int poison,
                      uint64_t n_out, double* out, int* err) {
  if (n_reads < 0 || raw_dtype < 0 || raw_dtype > 3 || W < 1 || W > 16 || !offs || !out || !err) return -1;
  if (n_reads && (!raw || !shift || !scale)) return -1;
  if (raw_dtype == 3 && n_reads && (!cal_offset || !cal_scale)) return -1;
  // everything the kernels index is inside what was handed in
  uint64_t max_len = 0;
  for (int r = 0; r < n_reads; ++r) {
    if (offs[r + 1] < offs[r]) return -1;
    max_len = std::max(max_len, offs[r + 1] - offs[r]);
  }
  const uint64_t total = offs[n_reads];
  if (n_out < total || total > (1ull << 31)) return -1;
  const size_t esz = raw_dtype == 0 ? 4 : raw_dtype == 2 ? 8 : 2;
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  };
  const size_t nr = (size_t)std::max(n_reads, 1);
  const size_t b_raw = std::max<size_t>(total * esz, 8), b_offs = (nr + 1) * 8, b_par = nr * 8, b_cal = nr * 4,
               b_norm = std::max<size_t>(total * (compute_f32 ? 4 : 8), 8), b_out = std::max<size_t>(n_out * 8, 8);
  void *d_raw = nullptr, *d_offs = nullptr, *d_shift = nullptr, *d_scale = nullptr, *d_co = nullptr, *d_cs = nullptr,
       *d_norm = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_raw, b_raw));
  if (ok) step(hipMalloc(&d_offs, b_offs));
  if (ok) step(hipMalloc(&d_shift, b_par));
  if (ok) step(hipMalloc(&d_scale, b_par));
  if (ok && raw_dtype == 3) step(hipMalloc(&d_co, b_cal));
  if (ok && raw_dtype == 3) step(hipMalloc(&d_cs, b_cal));
  if (ok) step(hipMalloc(&d_norm, b_norm));
  if (ok) step(hipMalloc(&d_out, b_out));
  if (ok && total) step(hipMemcpyAsync(d_raw, raw, total * esz, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_offs, offs, ((size_t)n_reads + 1) * 8, hipMemcpyHostToDevice, s));
  if (ok && n_reads) step(hipMemcpyAsync(d_shift, shift, (size_t)n_reads * 8, hipMemcpyHostToDevice, s));
  if (ok && n_reads) step(hipMemcpyAsync(d_scale, scale, (size_t)n_reads * 8, hipMemcpyHostToDevice, s));
  if (ok && n_reads && raw_dtype == 3) step(hipMemcpyAsync(d_co, cal_offset, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
  if (ok && n_reads && raw_dtype == 3) step(hipMemcpyAsync(d_cs, cal_scale, (size_t)n_reads * 4, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_norm, poison, b_norm, s));
  if (ok) step(hipMemsetAsync(d_out, poison, b_out, s));
  if (ok) {
    dynk::launch_preprocess(d_raw, raw_dtype, compute_f32, static_cast<const uint64_t*>(d_offs), static_cast<const double*>(d_shift),
                            static_cast<const double*>(d_scale), static_cast<const float*>(d_co), static_cast<const float*>(d_cs),
                            d_norm, static_cast<double*>(d_out), n_reads, max_len, W, n_sigmas, s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok && n_out) step(hipMemcpy(out, d_out, n_out * 8, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_out, d_norm, d_cs, d_co, d_scale, d_shift, d_offs, d_raw})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
