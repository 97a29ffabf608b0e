// rescale.hip -- test-only translation unit (tests/test_gpu_rescale_kernels.py): the product's rescale kernels
// (csrc/rescale.hip: k_rescale_init, k_rescale_fit, k_rescale_apply, launched by launch_rescale_init and launch_rescale_pass
// as launch.cpp launches them) run on borders, model means, signals and entry states the HOST hands in. Through whole
// alignments (tests/test_gpu_rescale.py) the guards' edges, the second 256-chunk pass of the row sums and the launch slices
// are out of reach; here every bit of the state, of the row means and of the signal is compared with the restatement
// (tests/rescale_chain.py).
//
// The product source is included, not copied: the kernels of its anonymous namespace are the ones that run.
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include <rescale.hip>  // csrc/rescale.hip by the include path (a quoted name would find this file)

using dynk::Emis;
using dynk::ReadDesc;
using dynk::ReadState;
using dynk::RescaleState;

static_assert(sizeof(RescaleState) == 32, "the test reads the state as (f8, f8, i4, i4, i4, i4)");

namespace {
constexpr size_t RSH_GUARD = 64;  // poisoned doubles behind sig and y
}

// n_desc descriptors in processing order (sig_off, par_off, seg_off, T, N, read per descriptor); status[n_state] indexed by
// `read`; rs[n_state]: in, the entry state of every read; out, what the pass left. rs_init[n_state]: what launch_rescale_init
// left in a poisoned array. sig0[n_sig]; sig[n_sig + RSH_GUARD]: in, the current signal; out, the signal after the pass and
// the poisoned guard. par_mean[n_par] (the other Emis fields hold NaN). segrow[n_seg]; y[n_seg + RSH_GUARD]: out, poisoned
// before the pass. max_T: what launch_rescale_pass sizes its grid by (0: the largest T of the descriptors).
// Every HIP call's hipError_t goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument.
// The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int rs_run(int n_desc, const uint64_t* sig_off, const uint64_t* par_off, const uint64_t* seg_off, const uint32_t* T,
                      const uint32_t* N, const uint32_t* read, int n_state, const int32_t* status, void* rs, void* rs_init,
                      uint64_t n_sig, const double* sig0, double* sig, uint64_t n_par, const double* par_mean, uint64_t n_seg,
                      const uint32_t* segrow, double* y, uint32_t max_T, int poison, int* err) {
  if (n_desc < 1 || n_state < 1 || n_sig < 1 || n_par < 1 || n_seg < 1) return -1;
  // everything the kernels index is inside what was handed in
  uint32_t big_T = 0;
  for (int k = 0; k < n_desc; ++k) {
    if (read[k] >= (uint32_t)n_state || T[k] < 2 || N[k] < 2) return -1;
    const uint64_t n = N[k] - 1;
    if (sig_off[k] > n_sig || (uint64_t)(T[k] - 1) > n_sig - sig_off[k]) return -1;
    if (seg_off[k] > n_seg || n > n_seg - seg_off[k]) return -1;
    if (par_off[k] > n_par || n > n_par - par_off[k]) return -1;
    uint32_t prev = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const uint32_t a = segrow[seg_off[k] + i];
      if (a < 1 || a >= T[k] || a <= prev) return -1;
      prev = a;
    }
    big_T = std::max(big_T, T[k]);
  }
  if (!max_T) max_T = big_T;
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  };
  std::vector<ReadDesc> descs((size_t)n_desc);
  for (int i = 0; i < n_desc; ++i) {  // the fields the rescale kernels do not read hold values no array has
    ReadDesc d{};
    d.sig_off = sig_off[i];
    d.par_off = par_off[i];
    d.path_off = 0x7fffffffffffff00ull;
    d.seg_off = seg_off[i];
    d.T = T[i];
    d.N = N[i];
    d.bw = 0x7fffffffu;
    d.read = read[i];
    d.ratio = -1.0;
    d.first_page = dynk::NO_PAGE;
    descs[(size_t)i] = d;
  }
  std::vector<ReadState> st((size_t)n_state);
  for (int i = 0; i < n_state; ++i) {
    ReadState s{};
    s.status = status[i];
    st[(size_t)i] = s;
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<Emis> par((size_t)n_par);
  for (uint64_t i = 0; i < n_par; ++i) par[(size_t)i] = Emis{par_mean[i], nan, nan, nan};
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState),
               b_rs = (size_t)n_state * sizeof(RescaleState), b_sig = n_sig * 8, b_sigg = (n_sig + RSH_GUARD) * 8,
               b_par = par.size() * sizeof(Emis), b_segrow = n_seg * 4, b_y = (n_seg + RSH_GUARD) * 8;
  void *d_descs = nullptr, *d_st = nullptr, *d_rs = nullptr, *d_sig0 = nullptr, *d_sig = nullptr, *d_par = nullptr,
       *d_segrow = nullptr, *d_y = nullptr;
  hipStream_t s = nullptr;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_st, b_st));
  if (ok) step(hipMalloc(&d_rs, b_rs));
  if (ok) step(hipMalloc(&d_sig0, b_sig));
  if (ok) step(hipMalloc(&d_sig, b_sigg));
  if (ok) step(hipMalloc(&d_par, b_par));
  if (ok) step(hipMalloc(&d_segrow, b_segrow));
  if (ok) step(hipMalloc(&d_y, b_y));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sig0, sig0, b_sig, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_sig, poison, b_sigg, s));
  if (ok) step(hipMemcpyAsync(d_sig, sig, b_sig, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_par, par.data(), b_par, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_y, poison, b_y, s));
  if (ok) step(hipMemsetAsync(d_rs, poison, b_rs, s));
  if (ok) {
    dynk::launch_rescale_init(static_cast<RescaleState*>(d_rs), (uint64_t)n_state, s);
    step(hipGetLastError());
  }
  if (ok) step(hipMemcpyAsync(rs_init, d_rs, b_rs, hipMemcpyDeviceToHost, s));
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpyAsync(d_rs, rs, b_rs, hipMemcpyHostToDevice, s));
  if (ok) {
    const dynk::TraceBuffers tb{nullptr, nullptr, static_cast<uint32_t*>(d_segrow), nullptr, nullptr};
    dynk::launch_rescale_pass(static_cast<const ReadDesc*>(d_descs), n_desc, max_T, static_cast<const ReadState*>(d_st), tb,
                              static_cast<const double*>(d_sig0), static_cast<double*>(d_sig), static_cast<const Emis*>(d_par),
                              static_cast<double*>(d_y), static_cast<RescaleState*>(d_rs), s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(rs, d_rs, b_rs, hipMemcpyDeviceToHost));
  if (ok) step(hipMemcpy(sig, d_sig, b_sigg, hipMemcpyDeviceToHost));
  if (ok) step(hipMemcpy(y, d_y, b_y, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_y, d_segrow, d_par, d_sig, d_sig0, d_rs, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
