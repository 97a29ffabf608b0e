// site_histogram.hip -- test-only translation unit (tests/test_gpu_site_histogram.py): the product's per-site summary kernels
// with the histograms on (site_summary_kernels.hpp, launched by launch_site_summary_kernels exactly as launch_site_summary
// launches them) over a signal pool, borders and per-row site ids the HOST hands in, and the product's quantile kernel
// (site_quantile_kernels.hpp, launched by launch_site_quantiles_kernel as launch_site_quantiles launches it) over histograms the
// host hands in (tests/site_histogram_cases.py). Every counter and every output integer is compared with a restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "site_quantile_kernels.hpp"
#include "site_summary_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;

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

// The arguments of ss_run (tests/device_math/site_summary.hip), and the histograms: bins / lo / hi as
// dyn_aligner_set_site_histogram takes them (inv_w is formed here as the host forms it), hist_on = 0 hands the kernels
// hist = nullptr. hist[num_sites * (bins + 18)] is uploaded as the counters' initial content (zeros, or a poison that must
// survive a run with hist_on = 0) and comes back as the device holds it after `runs` launches; acc[7 * num_sites + 5] likewise
// (zeroed on the device). Every HIP call's hipError_t goes into err[] in order (at most 64); returns how many were made, or -1
// for a bad argument. The first failing step ends the run (what was allocated is still freed).
extern "C" int sh_run(int n_desc, const uint64_t* sig_off, const uint64_t* par_off, const uint64_t* seg_off, const uint32_t* T,
                      const uint32_t* N, const uint32_t* read, int n_state, const int32_t* status, uint64_t n_sig,
                      const double* sig, uint64_t n_seg, const uint32_t* segrow, uint64_t n_par, const uint32_t* sites,
                      uint32_t num_sites, uint32_t read_lo, uint32_t read_hi, int runs, int bins, double lo, double hi, int hist_on,
                      uint64_t* acc, uint32_t* hist, int* err) {
  if (n_desc < 1 || n_state < 1 || n_sig < 1 || n_seg < 1 || n_par < 1 || num_sites < 1 || num_sites == 0xFFFFFFFFu || runs < 1 || runs > 4) return -1;
  if (bins < 2 || bins > dynk::SH_BINS_MAX || !std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi) || !hist || !acc) return -1;
  const double inv_w = (double)bins / (hi - lo);
  if (!std::isfinite(inv_w) || !(inv_w > 0.0)) return -1;
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
  Steps step{err};
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
  void *d_descs = nullptr, *d_st = nullptr, *d_sig = nullptr, *d_segrow = nullptr, *d_sites = nullptr, *d_acc = nullptr, *d_hist = nullptr;
  hipStream_t s = nullptr;
  const size_t H = (size_t)bins + 2 + dynk::SH_DWELL_BINS;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_sig = n_sig * 8,
               b_segrow = n_seg * 4, b_sites = n_par * 4, b_acc = ((size_t)num_sites * dynk::SS_FIELDS + dynk::SS_TOTALS) * 8,
               b_hist = (size_t)num_sites * H * 4;
  if (step.ok) step(hipStreamCreate(&s));
  if (step.ok) step(hipMalloc(&d_descs, b_descs));
  if (step.ok) step(hipMalloc(&d_st, b_st));
  if (step.ok) step(hipMalloc(&d_sig, b_sig));
  if (step.ok) step(hipMalloc(&d_segrow, b_segrow));
  if (step.ok) step(hipMalloc(&d_sites, b_sites));
  if (step.ok) step(hipMalloc(&d_acc, b_acc));
  if (step.ok) step(hipMalloc(&d_hist, b_hist));
  if (step.ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_sig, sig, b_sig, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_sites, sites, b_sites, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_hist, hist, b_hist, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemsetAsync(d_acc, 0, b_acc, s));
  if (step.ok) {
    unsigned long long* a = static_cast<unsigned long long*>(d_acc);
    dynk::SiteSummary ss{static_cast<const double*>(d_sig), static_cast<const uint32_t*>(d_sites), a,
                         a + (size_t)num_sites * dynk::SS_FIELDS, num_sites, read_lo, read_hi};
    if (hist_on) {
      ss.hist = static_cast<unsigned int*>(d_hist);
      ss.bins = (uint32_t)bins;
      ss.hist_lo = lo;
      ss.inv_w = inv_w;
    }
    for (int r = 0; r < runs; ++r)
      dynk::launch_site_summary_kernels(static_cast<const ReadDesc*>(d_descs), n_desc, max_N, static_cast<const ReadState*>(d_st),
                                        static_cast<const uint32_t*>(d_segrow), ss, s);
    step(hipGetLastError());
  }
  if (step.ok) step(hipStreamSynchronize(s));
  if (step.ok) step(hipMemcpy(acc, d_acc, b_acc, hipMemcpyDeviceToHost));
  if (step.ok) step(hipMemcpy(hist, d_hist, b_hist, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_hist, d_acc, d_sites, d_segrow, d_sig, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return step.k;
}

// k_site_quantiles over the sites [site_lo, site_hi) of a table[n_sites][bins + 18] the host hands in. out holds
// (1 + 4 * n_probs) * (site_hi - site_lo) uint32, pre-filled by the caller: n, then rank, bin, below, in_bin as [sites][n_probs]
// each, as the product's staging buffer holds them. One word more is allocated behind the output on the device and must come
// back as it went in (*guard). err[] and the return value as above.
extern "C" int sq_run(uint32_t n_sites, int bins, const uint32_t* table, uint32_t site_lo, uint32_t site_hi, const double* probs,
                      int n_probs, uint32_t* out, uint32_t* guard, int* err) {
  if (n_sites < 1 || bins < 2 || bins > dynk::SH_BINS_MAX || !table || site_lo > site_hi || site_hi > n_sites || !probs || n_probs < 1 ||
      n_probs > dynk::SQ_PROBS_MAX || !out || !guard)
    return -1;
  for (int q = 0; q < n_probs; ++q)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return -1;
  const size_t H = (size_t)bins + 2 + dynk::SH_DWELL_BINS, cnt = site_hi - site_lo;
  const size_t b_table = (size_t)n_sites * H * 4, words = (1 + 4 * (size_t)n_probs) * cnt, b_out = (words + 1) * 4;
  Steps step{err};
  void *d_table = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  std::vector<uint32_t> h(words + 1);
  std::copy(out, out + words, h.begin());
  h[words] = *guard;
  if (step.ok) step(hipStreamCreate(&s));
  if (step.ok) step(hipMalloc(&d_table, b_table));
  if (step.ok) step(hipMalloc(&d_out, b_out));
  if (step.ok) step(hipMemcpyAsync(d_table, table, b_table, hipMemcpyHostToDevice, s));
  if (step.ok) step(hipMemcpyAsync(d_out, h.data(), b_out, hipMemcpyHostToDevice, s));
  if (step.ok) {
    dynk::SiteQuantiles sq{};
    sq.hist = static_cast<const unsigned int*>(d_table) + H * site_lo;
    sq.bins = (uint32_t)bins;
    sq.count = (uint32_t)cnt;
    sq.n_probs = n_probs;
    for (int q = 0; q < n_probs; ++q) sq.probs[q] = probs[q];
    sq.out = static_cast<uint32_t*>(d_out);
    dynk::launch_site_quantiles_kernel(sq, s);
    step(hipGetLastError());
  }
  if (step.ok) step(hipStreamSynchronize(s));
  if (step.ok) step(hipMemcpy(h.data(), d_out, b_out, hipMemcpyDeviceToHost));
  if (step.ok) {
    std::copy(h.begin(), h.begin() + (long)words, out);
    *guard = h[words];
  }
  for (void* p : {d_out, d_table})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return step.k;
}
