// site_summary.hip -- test-only translation unit (tests/test_gpu_site_summary.py): the product's per-site summary kernels
// (site_summary_kernels.hpp: k_ssum_short, k_ssum_long, launched by launch_site_summary_kernels exactly as
// launch_site_summary launches them) run on a signal pool, borders and per-row site ids the HOST hands in
// (tests/site_summary_cases.py). Every integer of the table is compared with a Python-int restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "site_summary_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;

// n_desc descriptors in processing order (sig_off, par_off, seg_off, T, N, read per descriptor); status[n_state] indexed by
// `read`; sig[n_sig]; segrow[n_seg]; sites[n_par] (any uint32: the kernels check an id against num_sites before they use it).
// The table (7 * num_sites + 5 u64, zeroed on the device) takes `runs` launches of the reads [read_lo, read_hi) and comes back
// in acc[] as the device holds it: [num_sites][7], then the totals.
// Every HIP call's hipError_t goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument.
// The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int ss_run(int n_desc, const uint64_t* sig_off, const uint64_t* par_off, const uint64_t* seg_off, const uint32_t* T,
                      const uint32_t* N, const uint32_t* read, int n_state, const int32_t* status, uint64_t n_sig,
                      const double* sig, uint64_t n_seg, const uint32_t* segrow, uint64_t n_par, const uint32_t* sites,
                      uint32_t num_sites, uint32_t read_lo, uint32_t read_hi, int runs, uint64_t* acc, int* err) {
  if (n_desc < 1 || n_state < 1 || n_sig < 1 || n_seg < 1 || n_par < 1 || num_sites < 1 || num_sites == 0xFFFFFFFFu || runs < 1 || runs > 4) return -1;
  // everything the kernels index is inside what was handed in
  uint32_t max_N = 0;
  for (int k = 0; k < n_desc; ++k) {
    if (read[k] >= (uint32_t)n_state || T[k] < 2 || N[k] < 2) return -1;
    const uint64_t segs = N[k] - 1;
    if (seg_off[k] + segs > n_seg || par_off[k] + segs > n_par || sig_off[k] + (T[k] - 1) > n_sig) return -1;
    uint32_t prev = 0;
    for (uint64_t i = 0; i < segs; ++i) {
      const uint32_t a = segrow[seg_off[k] + i];
      if (a < 1 || a >= T[k] || a <= prev) return -1;
      prev = a;
    }
    max_N = std::max(max_N, N[k]);
  }
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  };
  std::vector<ReadDesc> descs((size_t)n_desc);
  for (int i = 0; i < n_desc; ++i) {  // launch.cpp: the fields these kernels do not read hold values no array has
    ReadDesc d{};
    d.sig_off = sig_off[i];
    d.par_off = par_off[i];
    d.path_off = 0x7fffffffffffff00ull;
    d.seg_off = seg_off[i];
    d.T = T[i];
    d.N = N[i];
    d.bw = 0x7fffffffu;
    d.read = read[i];
    d.ratio = (double)N[i] / (double)T[i];
    d.first_page = dynk::NO_PAGE;
    descs[(size_t)i] = d;
  }
  std::vector<ReadState> st((size_t)n_state);
  for (int i = 0; i < n_state; ++i) {
    ReadState s{};
    s.status = status[i];
    st[(size_t)i] = s;
  }
  void *d_descs = nullptr, *d_st = nullptr, *d_sig = nullptr, *d_segrow = nullptr, *d_sites = nullptr, *d_acc = nullptr;
  hipStream_t s = nullptr;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_sig = n_sig * 8,
               b_segrow = n_seg * 4, b_sites = n_par * 4, b_acc = ((size_t)num_sites * dynk::SS_FIELDS + dynk::SS_TOTALS) * 8;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_st, b_st));
  if (ok) step(hipMalloc(&d_sig, b_sig));
  if (ok) step(hipMalloc(&d_segrow, b_segrow));
  if (ok) step(hipMalloc(&d_sites, b_sites));
  if (ok) step(hipMalloc(&d_acc, b_acc));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sig, sig, b_sig, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sites, sites, b_sites, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_acc, 0, b_acc, s));
  if (ok) {
    unsigned long long* a = static_cast<unsigned long long*>(d_acc);
    const dynk::SiteSummary ss{static_cast<const double*>(d_sig), static_cast<const uint32_t*>(d_sites), a,
                               a + (size_t)num_sites * dynk::SS_FIELDS, num_sites, read_lo, read_hi};
    for (int r = 0; r < runs; ++r)
      dynk::launch_site_summary_kernels(static_cast<const ReadDesc*>(d_descs), n_desc, max_N, static_cast<const ReadState*>(d_st),
                                        static_cast<const uint32_t*>(d_segrow), ss, s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(acc, d_acc, b_acc, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_acc, d_sites, d_segrow, d_sig, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
