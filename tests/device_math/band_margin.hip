// band_margin.hip -- test-only translation unit (tests/test_gpu_band_margin.py): the product's band-margin kernels
// (band_margin_kernels.hpp: k_bmargin_init, k_bmargin, launched by launch_band_margin_kernels exactly as launch_band_margin
// launches them) run on descriptors and borders the HOST hands in (tests/band_margin_cases.py). Every integer is compared
// with a Python-int restatement of the all-rows definition.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "band_margin_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;

// n_desc descriptors in processing order (seg_off, T, N, bw, ratio, read per descriptor); status[n_state] indexed by `read`;
// segrow[n_seg]. out[3 * n_state] (low | high | edge_rows) is filled with `fill` on the device, takes `runs` launches of the
// reads [read_lo, read_hi) and comes back as the device holds it. Every HIP call's hipError_t goes into err[] in order (at most
// 64); returns how many were made, or -1 for a bad argument. The first failing step ends the run (what was allocated is still
// freed, those results are recorded too).
extern "C" int bm_run(int n_desc, const uint64_t* seg_off, const uint32_t* T, const uint32_t* N, const uint32_t* bw,
                      const double* ratio, const uint32_t* read, int n_state, const int32_t* status, uint64_t n_seg,
                      const uint32_t* segrow, uint32_t read_lo, uint32_t read_hi, int runs, uint32_t fill, uint32_t* out, int* err) {
  if (n_desc < 1 || n_state < 1 || n_seg < 1 || runs < 1 || runs > 4 || read_lo > read_hi || read_hi > (uint32_t)n_state) return -1;
  // everything the kernels index is inside what was handed in, and no sum of theirs leaves an int
  uint32_t max_N = 0;
  for (int k = 0; k < n_desc; ++k) {
    if (read[k] >= (uint32_t)n_state || T[k] < 2 || N[k] < 2 || T[k] > (1u << 24) || N[k] > T[k] || bw[k] > N[k]) return -1;
    if (!(ratio[k] > 0.0 && ratio[k] <= 1.0)) return -1;
    const uint64_t segs = N[k] - 1;
    if (seg_off[k] + segs > n_seg) return -1;
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
    d.sig_off = 0x7fffffffffffff00ull;
    d.par_off = 0x7fffffffffffff00ull;
    d.path_off = 0x7fffffffffffff00ull;
    d.seg_off = seg_off[i];
    d.T = T[i];
    d.N = N[i];
    d.bw = bw[i];
    d.read = read[i];
    d.ratio = ratio[i];
    d.first_page = dynk::NO_PAGE;
    descs[(size_t)i] = d;
  }
  std::vector<ReadState> st((size_t)n_state);
  for (int i = 0; i < n_state; ++i) {
    ReadState s{};
    s.status = status[i];
    st[(size_t)i] = s;
  }
  std::vector<uint32_t> filled((size_t)3 * n_state, fill);
  void *d_descs = nullptr, *d_st = nullptr, *d_segrow = nullptr, *d_out = nullptr;
  hipStream_t s = nullptr;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_segrow = n_seg * 4,
               b_out = filled.size() * 4;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_st, b_st));
  if (ok) step(hipMalloc(&d_segrow, b_segrow));
  if (ok) step(hipMalloc(&d_out, b_out));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_out, filled.data(), b_out, hipMemcpyHostToDevice, s));
  if (ok) {
    uint32_t* m = static_cast<uint32_t*>(d_out);
    const dynk::BandMargin bm{m, m + n_state, m + 2 * (size_t)n_state, read_lo, read_hi};
    for (int r = 0; r < runs; ++r)
      dynk::launch_band_margin_kernels(static_cast<const ReadDesc*>(d_descs), n_desc, max_N, static_cast<const ReadState*>(d_st),
                                       static_cast<const uint32_t*>(d_segrow), bm, s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(out, d_out, b_out, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_out, d_segrow, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
