// segment_scores.hip -- test-only translation unit (tests/test_gpu_segment_scores.py): the product's segment-score kernels
// (segment_score_kernels.hpp, launched by launch_segment_score_kernels exactly as launch_segment_scores launches them) run
// on borders the HOST hands in, so that window and segment lengths, ties and read ends are the test's choice and every
// output bit can be compared with the NumPy restatement of the definition (tests/segment_scores_cases.py).
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "segment_score_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;

// n_desc descriptors in processing order (sig_off, seg_off, path_off, T, N, read per descriptor); status[n_state] indexed by
// `read`; sig [n_sig]; pathn [rows_total]; segrow [n_seg]. The four columns (median_delta, mad_delta, homogeneity and the
// kernels' scratch) have n_out >= n_seg rows each (what lies beyond n_seg is a guard); they are filled with the byte `fill`
// on the device before the launches -- the product fills them with 0 -- and the first three are copied back after them into
// out[3 * n_out]. Every HIP call's hipError_t goes into err[] in order (at most 64); returns how many were made, or -1 for a
// bad argument. The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int ss_run(int n_desc, const uint64_t* sig_off, const uint64_t* seg_off, const uint64_t* path_off, const uint32_t* T,
                      const uint32_t* N, const uint32_t* read, int n_state, const int32_t* status, uint64_t n_sig,
                      const double* sig, uint64_t rows_total, const uint32_t* pathn, uint64_t n_seg, const uint32_t* segrow,
                      int window, int fill, uint64_t n_out, double* out, int* err) {
  if (n_desc < 1 || n_state < 1 || n_sig < 1 || rows_total < 1 || n_seg < 1 || n_out < n_seg) return -1;
  if (window < 1 || window > dynk::SC_MAX_WINDOW) return -1;
  // everything the kernels index is inside what was handed in
  uint32_t max_N = 0;
  for (int k = 0; k < n_desc; ++k) {
    if (read[k] >= (uint32_t)n_state || T[k] < 2 || N[k] < 2) return -1;
    if (path_off[k] + T[k] > rows_total || seg_off[k] + (N[k] - 1) > n_seg || sig_off[k] + (T[k] - 1) > n_sig) return -1;
    if (k > 0 && path_off[k] < path_off[k - 1] + T[k - 1]) return -1;
    uint32_t prev = 0;
    for (uint32_t i = 0; i + 1 < N[k]; ++i) {
      const uint32_t a = segrow[seg_off[k] + i];
      if (a < 1 || a >= T[k] || a <= prev) return -1;
      prev = a;
    }
    for (uint32_t t = 1; t < T[k]; ++t) {
      const uint32_t n = pathn[path_off[k] + t] & 0x7fffffffu;
      if (n < 1 || n >= N[k]) return -1;
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
    d.par_off = 0x7fffffffffffff00ull;
    d.path_off = path_off[i];
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
  void *d_descs = nullptr, *d_st = nullptr, *d_sig = nullptr, *d_pathn = nullptr, *d_segrow = nullptr, *d_cols = nullptr;
  hipStream_t s = nullptr;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_sig = n_sig * 8,
               b_pathn = rows_total * 4, b_segrow = n_seg * 4, b_cols = n_out * 32;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_st, b_st));
  if (ok) step(hipMalloc(&d_sig, b_sig));
  if (ok) step(hipMalloc(&d_pathn, b_pathn));
  if (ok) step(hipMalloc(&d_segrow, b_segrow));
  if (ok) step(hipMalloc(&d_cols, b_cols));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sig, sig, b_sig, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_pathn, pathn, b_pathn, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_cols, fill, b_cols, s));
  if (ok) {
    double* c = static_cast<double*>(d_cols);
    const dynk::ScoreCols sc{static_cast<const double*>(d_sig), c, c + n_out, c + 2 * n_out, c + 3 * n_out, window};
    dynk::launch_segment_score_kernels(static_cast<const ReadDesc*>(d_descs), n_desc, rows_total, max_N,
                                       static_cast<const ReadState*>(d_st), static_cast<const uint32_t*>(d_pathn),
                                       static_cast<const uint32_t*>(d_segrow), sc, s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(out, d_cols, n_out * 24, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_cols, d_segrow, d_pathn, d_sig, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
