// site_compare.hip -- test-only translation unit (tests/test_gpu_site_compare.py): the product's comparison kernel and the
// product's add kernel (site_compare_kernels.hpp, launched by launch_site_compare_kernel / launch_site_add_kernel as
// launch_site_compare / launch_site_add launch them) over histograms, tables and columns the HOST hands in
// (tests/site_compare_cases.py). Every output integer is compared with a restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "site_compare_kernels.hpp"

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

// k_site_compare over the pairs (site_lo + i, other_lo + i), i < count, of a table[n_sites][bins + 18] the host hands in. out
// holds 10 * count uint32 (SC_PAIR_BYTES per pair), pre-filled by the caller, in the layout of the product's staging buffer:
// level_num, dwell_num as uint64 [count], then n_a, n_b, level_at, dwell_at, level_side, dwell_side as uint32 [count]. One 64-bit
// word more is allocated behind the output on the device and must come back as it went in (*guard). Every HIP call's hipError_t
// goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument. The first failing step ends the
// run (what was allocated is still freed).
extern "C" int sc_run(uint32_t n_sites, int bins, const uint32_t* table, uint32_t site_lo, uint32_t other_lo, uint32_t count,
                      uint32_t* out, uint64_t* guard, int* err) {
  if (n_sites < 1 || bins < 2 || bins > dynk::SH_BINS_MAX || !table || count < 1 || !out || !guard) return -1;
  // both windows end inside the table: the kernel indexes nothing else
  if (site_lo > n_sites || count > n_sites - site_lo || other_lo > n_sites || count > n_sites - other_lo) return -1;
  const size_t H = (size_t)bins + 2 + dynk::SH_DWELL_BINS;
  const size_t b_table = (size_t)n_sites * H * 4, b_res = (size_t)dynk::SC_PAIR_BYTES * count, b_out = b_res + 8;
  Steps step{err};
  void *d_table = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  std::vector<unsigned char> h(b_out);
  std::memcpy(h.data(), out, b_res);
  std::memcpy(h.data() + b_res, guard, 8);
  if (step.ok) step(hipStreamCreate(&s));
  if (step.ok) step(hipMalloc(&d_table, b_table));
  if (step.ok) step(hipMalloc(&d_out, b_out));
  if (step.ok) step(hipMemcpyAsync(d_table, table, b_table, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_out, h.data(), b_out, hipMemcpyHostToDevice, s));
  if (step.ok) {
    dynk::SiteCompare sc{};
    sc.hist_a = static_cast<const unsigned int*>(d_table) + H * site_lo;
    sc.hist_b = static_cast<const unsigned int*>(d_table) + H * other_lo;
    sc.bins = (uint32_t)bins;
    sc.count = count;
    sc.out = static_cast<unsigned long long*>(d_out);
    dynk::launch_site_compare_kernel(sc, s);
    step(hipGetLastError());
  }
  if (step.ok) step(hipStreamSynchronize(s));
  if (step.ok) step(hipMemcpy(h.data(), d_out, b_out, hipMemcpyDeviceToHost));
  if (step.ok) {
    std::memcpy(out, h.data(), b_res);
    std::memcpy(guard, h.data() + b_res, 8);
  }
  for (void* p : {d_out, d_table})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return step.k;
}

// k_site_add: cols[count][7] (and counters[count][bins + 18] when hist_on) added into the sites [lo, lo + count) of
// acc[7 * n_sites + 5] and hist[n_sites][bins + 18], which are uploaded as the table's and the counters' initial content and come
// back as the device holds them afterwards. totals (5, or NULL: none) go to acc's last five words. hist_on = 0 hands the kernel
// hist = nullptr: a poisoned buffer must come back untouched. err[] and the return value as above.
extern "C" int sa_run(uint32_t n_sites, int bins, uint32_t lo, uint32_t count, const uint64_t* cols, const uint64_t* totals,
                      int hist_on, const uint32_t* counters, uint64_t* acc, uint32_t* hist, int* err) {
  if (n_sites < 1 || bins < 2 || bins > dynk::SH_BINS_MAX || count < 1 || lo > n_sites || count > n_sites - lo || !cols || !acc || !hist ||
      (hist_on && !counters))
    return -1;
  const size_t H = (size_t)bins + 2 + dynk::SH_DWELL_BINS, F = dynk::SS_FIELDS;
  const size_t b_acc = ((size_t)n_sites * F + dynk::SS_TOTALS) * 8, b_hist = (size_t)n_sites * H * 4, b_cols = (size_t)count * F * 8,
               b_cnt = (size_t)count * H * 4;
  Steps step{err};
  void *d_acc = nullptr, *d_hist = nullptr, *d_cols = nullptr, *d_cnt = nullptr;
  hipStream_t s = nullptr;
  if (step.ok) step(hipStreamCreate(&s));
  if (step.ok) step(hipMalloc(&d_acc, b_acc));
  if (step.ok) step(hipMalloc(&d_hist, b_hist));
  if (step.ok) step(hipMalloc(&d_cols, b_cols));
  if (step.ok) step(hipMalloc(&d_cnt, b_cnt));
  if (step.ok) step(hipMemcpyAsync(d_acc, acc, b_acc, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_hist, hist, b_hist, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_cols, cols, b_cols, hipMemcpyHostToDevice, s));
  if (step.ok && hist_on) step(hipMemcpyAsync(d_cnt, counters, b_cnt, hipMemcpyHostToDevice, s));
  if (step.ok) {
    dynk::SiteAdd sa{};
    sa.acc = static_cast<unsigned long long*>(d_acc) + F * lo;
    sa.totals = static_cast<unsigned long long*>(d_acc) + F * n_sites;
    sa.cols = static_cast<const unsigned long long*>(d_cols);
    sa.count = count;
    sa.width = (uint32_t)H;
    if (hist_on) {
      sa.hist = static_cast<unsigned int*>(d_hist) + H * lo;
      sa.counters = static_cast<const unsigned int*>(d_cnt);
    }
    sa.add_totals = totals ? 1 : 0;
    for (int f = 0; f < dynk::SS_TOTALS; ++f) sa.totals_in[f] = totals ? totals[f] : 0ull;
    dynk::launch_site_add_kernel(sa, s);
    step(hipGetLastError());
  }
  if (step.ok) step(hipStreamSynchronize(s));
  if (step.ok) step(hipMemcpy(acc, d_acc, b_acc, hipMemcpyDeviceToHost));
  if (step.ok) step(hipMemcpy(hist, d_hist, b_hist, hipMemcpyDeviceToHost));
  for (void* p : {d_cnt, d_cols, d_hist, d_acc})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return step.k;
}
