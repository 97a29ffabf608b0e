// site_calls.hip -- test-only translation unit (tests/test_gpu_site_calls.py, tests/test_site_call_host.py): the product's per-read
// site-call kernels (site_call_kernels.hpp: k_scall_short, k_scall_long, launched by launch_site_call_kernels exactly as
// launch_site_calls launches them) and the model's scatter kernel run on a signal pool, borders, per-row site ids and model rows
// the HOST hands in (tests/site_call_cases.py). Every double of the two columns is compared by its bits with a restatement.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "site_call_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;

// n_desc descriptors in processing order (sig_off, par_off, seg_off, T, N, read per descriptor); status[n_state] indexed by
// `read`; sig[n_sig]; segrow[n_seg]; sites[n_par] (any uint32: the kernels check an id against num_sites before they use it).
// The model: capacity == 0 is a dense table of num_sites rows, capacity > 0 a sparse one of `capacity` rows behind an empty map;
// it is zeroed, then the n_win windows (win_lo[w], win_count[w], their rows concatenated in rows[][5]) are uploaded one after the
// other -- dense: a copy into rows win_lo .., sparse: k_site_model_scatter -- and the call kernels run over the reads [read_lo,
// read_hi). out holds 2 * n_seg doubles [site_probability | site_z], pre-filled by the caller; one 64-bit word more is allocated
// behind it on the device and must come back as it went in (*guard). Sparse: keys_out[capacity] gets the map's keys and counts[3]
// n_keys after the uploads, n_keys after the call kernels, and the set rows that found no bucket.
// Every HIP call's hipError_t goes into err[] in order (at most 96); returns how many were made, or -1 for a bad argument.
// The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int sc_run(int n_desc, const uint64_t* sig_off, const uint64_t* par_off, const uint64_t* seg_off, const uint32_t* T,
                      const uint32_t* N, const uint32_t* read, int n_state, const int32_t* status, uint64_t n_sig, const double* sig,
                      uint64_t n_seg, const uint32_t* segrow, uint64_t n_par, const uint32_t* sites, uint32_t num_sites, uint32_t capacity,
                      int n_win, const uint32_t* win_lo, const uint32_t* win_count, const double* rows, uint32_t read_lo, uint32_t read_hi,
                      double* out, uint64_t* guard, uint32_t* keys_out, uint64_t* counts, int* err) {
  if (n_desc < 1 || n_state < 1 || n_sig < 1 || n_seg < 1 || n_par < 1 || num_sites < 1 || num_sites == 0xFFFFFFFFu || n_win < 0 || n_win > 8) return -1;
  if (!out || !guard || (capacity && (!keys_out || !counts))) return -1;
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
  uint64_t n_rows = 0;
  for (int w = 0; w < n_win; ++w) {
    if (win_lo[w] > num_sites || win_count[w] > num_sites - win_lo[w]) return -1;
    n_rows += win_count[w];
  }
  if (n_rows && !rows) return -1;
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
  const size_t F = (size_t)dynk::SC_MODEL_FIELDS;
  const size_t model_rows = capacity ? capacity : num_sites;
  void *d_descs = nullptr, *d_st = nullptr, *d_sig = nullptr, *d_segrow = nullptr, *d_sites = nullptr, *d_model = nullptr, *d_rows = nullptr,
       *d_keys = nullptr, *d_stats = nullptr, *d_out = nullptr, *d_exp = nullptr;
  hipStream_t s = nullptr;
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_sig = n_sig * 8, b_segrow = n_seg * 4,
               b_sites = n_par * 4, b_model = model_rows * F * 8, b_rows = std::max<size_t>(8, n_rows * F * 8), b_keys = std::max<size_t>(4, (size_t)capacity * 4),
               b_stats = 4 * 8, b_res = n_seg * 16, b_out = b_res + 8, b_exp = (size_t)dynmath::STRICT_EXP_WORDS * 8;
  std::vector<unsigned char> h(b_out);
  std::memcpy(h.data(), out, b_res);
  std::memcpy(h.data() + b_res, guard, 8);
  if (ok) step(hipStreamCreate(&s));
  for (auto [p, bytes] : {std::pair<void**, size_t>{&d_descs, b_descs}, {&d_st, b_st}, {&d_sig, b_sig}, {&d_segrow, b_segrow}, {&d_sites, b_sites},
                          {&d_model, b_model}, {&d_rows, b_rows}, {&d_keys, b_keys}, {&d_stats, b_stats}, {&d_out, b_out}, {&d_exp, b_exp}})
    if (ok) step(hipMalloc(p, bytes));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sig, sig, b_sig, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_segrow, segrow, b_segrow, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_sites, sites, b_sites, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_out, h.data(), b_out, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_exp, dynmath::strict_exp_table(), b_exp, hipMemcpyHostToDevice, s));
  if (ok && n_rows) step(hipMemcpyAsync(d_rows, rows, n_rows * F * 8, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_model, 0, b_model, s));
  if (ok) step(hipMemsetAsync(d_keys, 0xFF, b_keys, s));
  if (ok) step(hipMemsetAsync(d_stats, 0, b_stats, s));
  unsigned long long* stats = static_cast<unsigned long long*>(d_stats);  // [3] the map's statistics, [1] this run's dropped rows
  if (ok) {
    uint64_t o = 0;
    for (int w = 0; w < n_win && ok; ++w) {
      if (!win_count[w]) continue;
      const double* src = static_cast<const double*>(d_rows) + o * F;
      if (capacity) {
        dynk::SiteModelScatter ms{static_cast<uint32_t*>(d_keys), capacity, stats, static_cast<double*>(d_model), src, win_lo[w], win_count[w], stats + 3};
        dynk::launch_site_model_scatter_kernel(ms, s);
        step(hipGetLastError());
      } else {
        step(hipMemcpyAsync(static_cast<double*>(d_model) + (size_t)win_lo[w] * F, src, (size_t)win_count[w] * F * 8, hipMemcpyDeviceToDevice, s));
      }
      o += win_count[w];
    }
  }
  uint64_t h_stats[4] = {0, 0, 0, 0};
  if (ok && capacity) {
    step(hipStreamSynchronize(s));
    if (ok) step(hipMemcpy(h_stats, d_stats, b_stats, hipMemcpyDeviceToHost));
    counts[0] = h_stats[dynk::SM_N_KEYS];
    counts[2] = h_stats[3];
  }
  if (ok) {
    dynk::SiteCalls sc{};
    sc.sig = static_cast<const double*>(d_sig);
    sc.sites = static_cast<const uint32_t*>(d_sites);
    sc.model = static_cast<const double*>(d_model);
    sc.map_keys = capacity ? static_cast<const uint32_t*>(d_keys) : nullptr;
    sc.capacity = capacity;
    sc.num_sites = num_sites;
    sc.read_lo = read_lo;
    sc.read_hi = read_hi;
    sc.exp_tab = static_cast<const uint64_t*>(d_exp);
    sc.prob = static_cast<double*>(d_out);
    sc.z = static_cast<double*>(d_out) + n_seg;
    dynk::launch_site_call_kernels(static_cast<const ReadDesc*>(d_descs), n_desc, max_N, static_cast<const ReadState*>(d_st),
                                   static_cast<const uint32_t*>(d_segrow), sc, s);
    step(hipGetLastError());
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(h.data(), d_out, b_out, hipMemcpyDeviceToHost));
  if (ok && capacity) {
    step(hipMemcpy(h_stats, d_stats, b_stats, hipMemcpyDeviceToHost));
    if (ok) step(hipMemcpy(keys_out, d_keys, (size_t)capacity * 4, hipMemcpyDeviceToHost));
    counts[1] = h_stats[dynk::SM_N_KEYS];
  }
  if (ok) {
    std::memcpy(out, h.data(), b_res);
    std::memcpy(guard, h.data() + b_res, 8);
  }
  // frees are recorded whatever happened before
  for (void* p : {d_exp, d_out, d_stats, d_keys, d_rows, d_model, d_sites, d_segrow, d_sig, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}

// the home bucket of an id, as the kernels hash it: the test builds ids that share one
extern "C" uint32_t sc_home(uint32_t id, uint32_t capacity) { return dynk::sm_home(id, capacity); }
