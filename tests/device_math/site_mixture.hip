// site_mixture.hip -- test-only translation unit (tests/test_gpu_site_mixture.py): the product's mixture kernel
// (site_mixture_kernels.hpp, launched by launch_site_mixture_kernel as launch_site_mixture launches it) over a table of counters the
// HOST hands in (tests/site_mixture_cases.py). Every output, doubles by their bit patterns, is compared with a restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "site_mixture_kernels.hpp"

namespace {
struct Steps {
  int* err;
  int k = 0;
  bool ok = true;
  bool operator()(hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  }
};
}  // namespace

// k_site_mixture over the pairs (site_lo + i, other_lo + i), i < count, of a table[n_sites][bins + 18] the host hands in; other_lo =
// 0xFFFFFFFF: the single-sample form. The constants are formed from (lo, hi, tol) as dyn_aligner_site_mixture forms them. out holds
// 20 * count uint32 (SM_PAIR_BYTES per pair), pre-filled by the caller, in the layout of the product's staging buffer: pi1, mu0, mu1,
// var0, var1, r_a, r_b as float64 [count], then n_a, n_b, out_a, out_b, iters, status as uint32 [count]. One 64-bit word more is
// allocated behind the output on the device and must come back as it went in (*guard). Every HIP call's hipError_t goes into err[]
// in order (at most 64); returns how many were made, or -1 for a bad argument. The first failing step ends the run (what was
// allocated is still freed).
extern "C" int sm_run(uint32_t n_sites, int bins, const uint32_t* table, uint32_t site_lo, uint32_t other_lo, uint32_t count, double lo,
                      double hi, uint32_t max_iters, double tol, uint32_t min_n, uint32_t* out, uint64_t* guard, int* err) {
  if (n_sites < 1 || bins < 2 || bins > dynk::SH_BINS_MAX || !table || count < 1 || !out || !guard || !(lo < hi)) return -1;
  if (max_iters < 1 || max_iters > dynk::SM_MAX_ITERS || !(tol >= 0.0) || min_n < 2) return -1;
  const bool one = other_lo == 0xFFFFFFFFu;
  // both windows end inside the table: the kernel indexes nothing else
  if (site_lo > n_sites || count > n_sites - site_lo || (!one && (other_lo > n_sites || count > n_sites - other_lo))) return -1;
  const size_t H = (size_t)bins + 2 + dynk::SH_DWELL_BINS;
  const size_t b_table = (size_t)n_sites * H * 4, b_res = (size_t)dynk::SM_PAIR_BYTES * count, b_out = b_res + 8;
  const size_t b_exp = (size_t)dynmath::STRICT_EXP_WORDS * 8;
  Steps step{err};
  void *d_table = nullptr, *d_out = nullptr, *d_exp = nullptr;
  hipStream_t s = nullptr;
  std::vector<unsigned char> h(b_out);
  std::memcpy(h.data(), out, b_res);
  std::memcpy(h.data() + b_res, guard, 8);
  if (step.ok) step(hipStreamCreate(&s));
  if (step.ok) step(hipMalloc(&d_table, b_table));
  if (step.ok) step(hipMalloc(&d_out, b_out));
  if (step.ok) step(hipMalloc(&d_exp, b_exp));
  if (step.ok) step(hipMemcpyAsync(d_table, table, b_table, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_out, h.data(), b_out, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_exp, dynmath::strict_exp_table(), b_exp, hipMemcpyHostToDevice, s));
  if (step.ok) {
    dynk::SiteMixture sm{};
    sm.hist_a = static_cast<const unsigned int*>(d_table) + H * site_lo;
    sm.hist_b = one ? nullptr : static_cast<const unsigned int*>(d_table) + H * other_lo;
    sm.exp_tab = static_cast<const uint64_t*>(d_exp);
    sm.bins = (uint32_t)bins;
    sm.count = count;
    sm.max_iters = max_iters;
    sm.min_n = min_n;
    sm.lo = lo;
    sm.w = (hi - lo) / (double)bins;
    sm.vfloor = (sm.w * sm.w) / 12.0;
    sm.tol_mu = tol * sm.w;
    sm.tol_pi = tol;
    sm.out = static_cast<double*>(d_out);
    dynk::launch_site_mixture_kernel(sm, s);
    step(hipGetLastError());
  }
  if (step.ok) step(hipStreamSynchronize(s));
  if (step.ok) step(hipMemcpy(h.data(), d_out, b_out, hipMemcpyDeviceToHost));
  if (step.ok) {
    std::memcpy(out, h.data(), b_res);
    std::memcpy(guard, h.data() + b_res, 8);
  }
  for (void* p : {d_exp, d_out, d_table})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return step.k;
}
