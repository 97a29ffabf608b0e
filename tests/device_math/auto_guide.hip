// auto_guide.hip -- test-only translation unit (tests/test_gpu_auto_guide.py): the product's pre-pass kernel (k_auto_guide of
// dynamont_amd/csrc/auto_guide.hip, launched by launch_auto_guide exactly as dyn_batch_auto_guide launches it) run on
// descriptors, samples and emission entries the HOST hands in. Every guide entry is compared with the g++ build of the same
// header (tests/device_math/auto_guide_host.cpp).
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../dynamont_amd/csrc/auto_guide.hip"  // (this directory has a file of the same name)

using dynk::ReadDesc;

// n_desc reads in processing order (T, N, sig_off, par_off per descriptor) over n_sig samples and n_par emission entries
// (mean / stdev / neg_log_stdev). guide[n_sig] is filled with `fill` on the device, takes one launch over the first n_run
// descriptors (0: the empty range) with n_groups workgroups and comes back as the device holds it. Every HIP call's hipError_t
// goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument. The first failing step ends the
// run (what was allocated is still freed, those results are recorded too).
extern "C" int ag_run(int n_desc, const uint32_t* T, const uint32_t* N, const uint64_t* sig_off, const uint64_t* par_off,
                      uint64_t n_sig, const double* sig, uint64_t n_par, const double* mean, const double* stdev,
                      const double* neg_log_stdev, int hw, double m1, double e2, int n_run, int n_groups, int32_t fill, int32_t* guide,
                      int* err) {
  if (n_desc < 1 || n_sig < 1 || n_par < 1 || n_run < 0 || n_run > n_desc || n_groups < 1 || n_groups > 4096) return -1;
  if (hw < 1 || hw > dynk::WIDE_MAX_HALF_BAND) return -1;
  // everything the kernel indexes is inside what was handed in: T - 1 samples and guide entries at sig_off, N - 1 emission
  // entries at par_off
  for (int k = 0; k < n_desc; ++k) {
    if (T[k] < 1 || N[k] < 1 || T[k] > (1u << 24) || N[k] > (1u << 24)) return -1;
    if (sig_off[k] > n_sig || (uint64_t)(T[k] - 1) > n_sig - sig_off[k]) return -1;
    if (par_off[k] > n_par || (uint64_t)(N[k] - 1) > n_par - par_off[k]) return -1;
  }
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  };
  std::vector<ReadDesc> descs((size_t)n_desc);
  for (int i = 0; i < n_desc; ++i) {  // the fields the kernel does not read hold values no array has
    ReadDesc d{};
    d.sig_off = sig_off[i];
    d.par_off = par_off[i];
    d.path_off = 0x7fffffffffffff00ull;
    d.seg_off = 0x7fffffffffffff00ull;
    d.T = T[i];
    d.N = N[i];
    d.read = (uint32_t)i;
    d.first_page = dynk::NO_PAGE;
    descs[(size_t)i] = d;
  }
  std::vector<dynmath::Emis> par((size_t)n_par);
  for (uint64_t i = 0; i < n_par; ++i) par[(size_t)i] = dynmath::Emis{mean[i], 1.0 / stdev[i], neg_log_stdev[i], stdev[i]};
  std::vector<int32_t> filled((size_t)n_sig, fill);
  void *d_descs = nullptr, *d_sig = nullptr, *d_par = nullptr, *d_guide = nullptr, *d_head = nullptr;
  hipStream_t s = nullptr;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_sig = n_sig * 8, b_par = par.size() * sizeof(dynmath::Emis), b_guide = n_sig * 4;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_sig, b_sig));
  if (ok) step(hipMalloc(&d_par, b_par));
  if (ok) step(hipMalloc(&d_guide, b_guide));
  if (ok) step(hipMalloc(&d_head, 256));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sig, sig, b_sig, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_par, par.data(), b_par, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_guide, filled.data(), b_guide, hipMemcpyHostToDevice, s));
  if (ok) {
    dynk::AutoGuideArgs a{};
    a.descs = static_cast<const ReadDesc*>(d_descs);
    a.n_reads = n_run;
    a.bw = hw;
    a.sig = static_cast<const double*>(d_sig);
    a.par = static_cast<const dynmath::Emis*>(d_par);
    a.guide = static_cast<int32_t*>(d_guide);
    a.head = static_cast<uint32_t*>(d_head);
    a.m1 = m1;
    a.e2 = e2;
    step(dynk::launch_auto_guide(a, n_groups, s));
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(guide, d_guide, b_guide, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_head, d_guide, d_par, d_sig, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
