// segment_median.hip -- test-only translation unit (tests/test_gpu_segment_median.py): the product's per-segment kernels
// (segment_kernels.hpp: k_median, k_median_long, k_final, launched by launch_segment_medians exactly as launch_segments
// launches them) run on path arrays the HOST hands in. In the product pp[] is written by the traceback and never leaves the
// device, so the selection these kernels make can only be seen through a 1e-6 comparison of whole reads; here every output
// bit is compared with a sort.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "segment_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;
using dynk::SegRow;

static_assert(sizeof(SegRow) == 16, "the test reads rows as (uint32, uint32, double)");

// n_desc descriptors in processing order (path_off, seg_off, T, N, read per descriptor); status[n_state] indexed by `read`;
// pp / pathn [rows_total]; segrow [n_seg]. med_hi, med_lo [n_out] and rows [n_out] (n_out >= n_seg: what lies beyond n_seg is
// a guard) are filled with the byte `poison` on the device before the launches and copied back after them.
// Every HIP call's hipError_t goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument.
// The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int sm_run(int n_desc, const uint64_t* path_off, const uint64_t* seg_off, const uint32_t* T, const uint32_t* N,
                      const uint32_t* read, int n_state, const int32_t* status, uint64_t rows_total, const double* pp,
                      const uint32_t* pathn, uint64_t n_seg, const uint32_t* segrow, int kmer_size, int poison, uint64_t n_out,
                      double* med_hi, double* med_lo, void* rows, int* err) {
  if (n_desc < 0 || n_state < 1 || rows_total < 1 || n_seg < 1 || n_out < n_seg) return -1;
  // everything the kernels index is inside what was handed in
  uint32_t max_N = 0;
  for (int k = 0; k < n_desc; ++k) {
    if (read[k] >= (uint32_t)n_state || T[k] < 2 || N[k] < 2) return -1;
    if (path_off[k] + T[k] > rows_total || seg_off[k] + (N[k] - 1) > n_seg) return -1;
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
  std::vector<ReadDesc> descs((size_t)std::max(n_desc, 1));
  for (int i = 0; i < n_desc; ++i) {  // launch.cpp: the fields the per-segment kernels do not read hold values no array has
    ReadDesc d{};
    d.sig_off = d.par_off = 0x7fffffffffffff00ull;
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
  void *d_descs = nullptr, *d_st = nullptr, *d_pp = nullptr, *d_pathn = nullptr, *d_segrow = nullptr, *d_hi = nullptr,
       *d_lo = nullptr, *d_rows = nullptr;
  hipStream_t s = nullptr;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_pp = rows_total * 8,
               b_pathn = rows_total * 4, b_segrow = n_seg * 4, b_med = n_out * 8, b_rows = n_out * sizeof(SegRow);
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_st, b_st));
  if (ok) step(hipMalloc(&d_pp, b_pp));
  if (ok) step(hipMalloc(&d_pathn, b_pathn));
  if (ok) step(hipMalloc(&d_segrow, b_segrow));
  if (ok) step(hipMalloc(&d_hi, b_med));
  if (ok) step(hipMalloc(&d_lo, b_med));
  if (ok) step(hipMalloc(&d_rows, b_rows));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_pp, pp, b_pp, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_pathn, pathn, b_pathn, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_hi, poison, b_med, s));
  if (ok) step(hipMemsetAsync(d_lo, poison, b_med, s));
  if (ok) step(hipMemsetAsync(d_rows, poison, b_rows, s));
  if (ok) {
    const dynk::TraceBuffers tb{static_cast<double*>(d_pp), static_cast<uint32_t*>(d_pathn), static_cast<uint32_t*>(d_segrow),
                                static_cast<double*>(d_hi), static_cast<double*>(d_lo)};
    dynk::launch_segment_medians(static_cast<const ReadDesc*>(d_descs), n_desc, rows_total, max_N,
                                 static_cast<const ReadState*>(d_st), tb, static_cast<SegRow*>(d_rows), kmer_size, s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(med_hi, d_hi, b_med, hipMemcpyDeviceToHost));
  if (ok) step(hipMemcpy(med_lo, d_lo, b_med, hipMemcpyDeviceToHost));
  if (ok) step(hipMemcpy(rows, d_rows, b_rows, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_rows, d_lo, d_hi, d_segrow, d_pathn, d_pp, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
