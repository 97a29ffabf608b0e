// pool_stats.hip -- test-only translation unit (tests/test_gpu_pool_stats.py): the product's pooled Baum-Welch statistics
// (csrc/pool_stats.hip: k_pool_fill, k_pool_keys, rocPRIM's radix sort, k_pool_gather, k_pool_segments, launched by
// launch_pool_stats with buffers sized by pool_stats_work_bytes / pool_stats_temp_bytes, as dyn_batch_device_pooled does)
// run on descriptors, k-mer codes and per-column sums the HOST hands in. In the product the column sums are written by the
// training launch and never leave the device, so the association of the pooled sum can only be seen through whole reads;
// here every bit of pooled[] is compared with a restatement of the host's order (tests/pool_stats_cases.py).
//
// The product source is included, not copied: the kernels of its anonymous namespace are the ones that run.
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include <pool_stats.hip>  // csrc/pool_stats.hip by the include path (a quoted name would find this file)

using dynk::ReadDesc;
using dynk::ReadState;

namespace {
constexpr size_t PS_GUARD = 256;  // poisoned bytes behind the work and the temp buffer, poisoned doubles behind pooled
}

// n_desc descriptors in processing order (par_off, N, read per descriptor; the other fields get values no array has);
// status[n_state] indexed by `read`; kmers, col_w, col_s1, col_s2 [total_cols]; pooled[3 * num_kmers + PS_GUARD]: in, the
// initial contents (the guard is overwritten with the poison); out, what the device left. The work and temp buffers are
// filled with the byte `poison` before the launch; guard[2 * PS_GUARD] receives the bytes behind them afterwards.
// Every HIP call's hipError_t goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument.
// The first failing step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int ps_run(int n_desc, const uint64_t* par_off, const uint32_t* N, const uint32_t* read, int n_state,
                      const int32_t* status, uint64_t total_cols, const int32_t* kmers, const double* col_w, const double* col_s1,
                      const double* col_s2, uint64_t num_kmers, int poison, double* pooled, unsigned char* guard, int* err) {
  if (n_desc < 1 || n_state < 1 || total_cols < 1 || total_cols >= (1ull << 31) || num_kmers < 1 || num_kmers >= (1ull << 31))
    return -1;
  // everything the kernels index is inside what was handed in: columns inside [0, total_cols) and owned by one descriptor at
  // most, every code (of owned columns and of the others) inside [0, num_kmers)
  uint32_t max_N = 0;
  std::vector<unsigned char> owned((size_t)total_cols, 0);
  for (int k = 0; k < n_desc; ++k) {
    if (read[k] >= (uint32_t)n_state || N[k] < 1) return -1;
    if (par_off[k] > total_cols || (uint64_t)(N[k] - 1) > total_cols - par_off[k]) return -1;
    for (uint64_t c = 0; c + 1 < N[k]; ++c) {
      if (owned[(size_t)(par_off[k] + c)]) return -1;
      owned[(size_t)(par_off[k] + c)] = 1;
    }
    max_N = std::max(max_N, N[k]);
  }
  for (uint64_t i = 0; i < total_cols; ++i)
    if (kmers[i] < 0 || (uint64_t)kmers[i] >= num_kmers) return -1;
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  };
  std::vector<ReadDesc> descs((size_t)n_desc);
  for (int i = 0; i < n_desc; ++i) {  // the fields pool_stats does not read hold values no array has
    ReadDesc d{};
    d.sig_off = d.path_off = d.seg_off = 0x7fffffffffffff00ull;
    d.par_off = par_off[i];
    d.T = 0x7fffffffu;
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
  const size_t b_work = dynk::pool_stats_work_bytes(total_cols), b_temp = dynk::pool_stats_temp_bytes(total_cols, num_kmers);
  const size_t b_descs = descs.size() * sizeof(ReadDesc), b_st = st.size() * sizeof(ReadState), b_km = total_cols * 4,
               b_col = total_cols * 8, n_pooled = 3 * num_kmers, b_pooled = (n_pooled + PS_GUARD) * 8;
  void *d_descs = nullptr, *d_st = nullptr, *d_km = nullptr, *d_w = nullptr, *d_s1 = nullptr, *d_s2 = nullptr, *d_pooled = nullptr,
       *d_work = nullptr, *d_temp = nullptr;
  hipStream_t s = nullptr;
  if (ok) step(hipStreamCreate(&s));
  if (ok) step(hipMalloc(&d_descs, b_descs));
  if (ok) step(hipMalloc(&d_st, b_st));
  if (ok) step(hipMalloc(&d_km, b_km));
  if (ok) step(hipMalloc(&d_w, b_col));
  if (ok) step(hipMalloc(&d_s1, b_col));
  if (ok) step(hipMalloc(&d_s2, b_col));
  if (ok) step(hipMalloc(&d_pooled, b_pooled));
  if (ok) step(hipMalloc(&d_work, b_work + PS_GUARD));
  if (ok) step(hipMalloc(&d_temp, b_temp + PS_GUARD));
  if (ok) step(hipMemcpyAsync(d_descs, descs.data(), b_descs, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_st, st.data(), b_st, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_km, kmers, b_km, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_w, col_w, b_col, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_s1, col_s1, b_col, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemcpyAsync(d_s2, col_s2, b_col, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_pooled, poison, b_pooled, s));
  if (ok) step(hipMemcpyAsync(d_pooled, pooled, n_pooled * 8, hipMemcpyHostToDevice, s));
  if (ok) step(hipMemsetAsync(d_work, poison, b_work + PS_GUARD, s));
  if (ok) step(hipMemsetAsync(d_temp, poison, b_temp + PS_GUARD, s));
  if (ok) {
    const dynk::TrainBuffers tb{static_cast<double*>(d_w), static_cast<double*>(d_s1), static_cast<double*>(d_s2), nullptr};
    step(dynk::launch_pool_stats(static_cast<const ReadDesc*>(d_descs), n_desc, max_N, static_cast<const ReadState*>(d_st),
                                 static_cast<const int32_t*>(d_km), tb, static_cast<double*>(d_pooled), num_kmers, total_cols,
                                 d_work, d_temp, b_temp, s));
  }
  if (ok) step(hipStreamSynchronize(s));
  if (ok) step(hipMemcpy(pooled, d_pooled, b_pooled, hipMemcpyDeviceToHost));
  if (ok) step(hipMemcpy(guard, static_cast<char*>(d_work) + b_work, PS_GUARD, hipMemcpyDeviceToHost));
  if (ok) step(hipMemcpy(guard + PS_GUARD, static_cast<char*>(d_temp) + b_temp, PS_GUARD, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  for (void* p : {d_temp, d_work, d_pooled, d_s2, d_s1, d_w, d_km, d_st, d_descs})
    if (p) step(hipFree(p));
  if (s) step(hipStreamDestroy(s));
  return k;
}
