// site_map.hip -- test-only translation unit (tests/test_gpu_site_map.py, tests/test_site_map_host.py): the sparse mode of the
// per-site table on arrays the HOST hands in. The product's filling kernels (site_summary_kernels.hpp, launched by
// launch_site_summary_kernels exactly as launch_site_summary launches them) look their rows up in a map (site_map.hpp); the
// window kernels (site_map_kernels.hpp: k_site_gather, k_site_scatter_add, k_site_map_windows) read and add windows of ids.
// Every integer is compared with a Python-int restatement (tests/site_map_cases.py). sm_home is exported on the host side: the
// tests take home buckets from it and from nothing else.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes. Every call returns 0, a hipError_t, or -1 for an argument that would index outside what was handed in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "site_map_kernels.hpp"
#include "site_summary_kernels.hpp"

using dynk::ReadDesc;
using dynk::ReadState;

namespace {
struct Harness {
  uint32_t num_sites = 0, capacity = 0, bins = 0, width = 0;
  double lo = 0.0, inv_w = 0.0;
  uint32_t* keys = nullptr;
  unsigned long long* acc = nullptr;  // [7 capacity + 5 + 3]
  unsigned int* hist = nullptr;       // [capacity][width]; nullptr: bins == 0
  hipStream_t s = nullptr, s2 = nullptr;
  std::vector<void*> batch;           // the device arrays of the last smh_fill, freed with the next one
  size_t acc_words() const { return (size_t)capacity * dynk::SS_FIELDS + dynk::SS_TOTALS + dynk::SM_STATS; }
  unsigned long long* totals() const { return acc + (size_t)capacity * dynk::SS_FIELDS; }
  unsigned long long* stats() const { return totals() + dynk::SS_TOTALS; }
};

#define TRY(x)                             \
  do {                                     \
    const hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return (int)e_;  \
  } while (0)

int upload(Harness* h, void** d, const void* src, size_t bytes) {
  TRY(hipMalloc(d, std::max<size_t>(bytes, 8)));
  h->batch.push_back(*d);
  TRY(hipMemcpyAsync(*d, src, bytes, hipMemcpyHostToDevice, h->s));
  return 0;
}

int free_batch(Harness* h) {
  int rc = 0;
  for (void* p : h->batch) {
    const hipError_t e = hipFree(p);
    if (e != hipSuccess && !rc) rc = (int)e;
  }
  h->batch.clear();
  return rc;
}
}  // namespace

extern "C" uint32_t smh_home(uint32_t id, uint32_t capacity) { return dynk::sm_home(id, capacity); }
extern "C" void smh_home_many(const uint32_t* ids, uint64_t n, uint32_t capacity, uint32_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = dynk::sm_home(ids[i], capacity);
}
extern "C" uint32_t smh_probe_max() { return dynk::SM_PROBE_MAX; }

// an empty map of `capacity` rows over the ids below num_sites; bins > 0: histograms of bins + 2 + 16 counters per row
extern "C" int smh_create(uint32_t num_sites, uint32_t capacity, uint32_t bins, double lo, double inv_w, void** out) {
  if (!out || num_sites < 1 || num_sites == 0xFFFFFFFFu || capacity < 1 || capacity == 0xFFFFFFFFu || bins > (uint32_t)dynk::SH_BINS_MAX) return -1;
  Harness* h = new Harness();
  *out = h;
  h->num_sites = num_sites;
  h->capacity = capacity;
  h->bins = bins;
  h->width = bins ? bins + 2u + (uint32_t)dynk::SH_DWELL_BINS : 0u;
  h->lo = lo;
  h->inv_w = inv_w;
  TRY(hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking));
  TRY(hipStreamCreateWithFlags(&h->s2, hipStreamNonBlocking));
  TRY(hipMalloc(reinterpret_cast<void**>(&h->keys), (size_t)capacity * 4));
  TRY(hipMalloc(reinterpret_cast<void**>(&h->acc), h->acc_words() * 8));
  if (bins) TRY(hipMalloc(reinterpret_cast<void**>(&h->hist), (size_t)capacity * h->width * 4));
  TRY(hipMemsetAsync(h->keys, 0xFF, (size_t)capacity * 4, h->s));
  TRY(hipMemsetAsync(h->acc, 0, h->acc_words() * 8, h->s));
  if (bins) TRY(hipMemsetAsync(h->hist, 0, (size_t)capacity * h->width * 4, h->s));
  TRY(hipStreamSynchronize(h->s));
  return 0;
}

extern "C" int smh_destroy(void* hv) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h) return -1;
  int rc = free_batch(h);
  for (void* p : {(void*)h->keys, (void*)h->acc, (void*)h->hist})
    if (p) {
      const hipError_t e = hipFree(p);
      if (e != hipSuccess && !rc) rc = (int)e;
    }
  for (hipStream_t s : {h->s, h->s2})
    if (s) {
      const hipError_t e = hipStreamDestroy(s);
      if (e != hipSuccess && !rc) rc = (int)e;
    }
  delete h;
  return rc;
}

// `runs` launches of the reads [read_lo, read_hi) of a batch laid out as tests/device_math/site_summary.hip takes it. sync == 0:
// the launches are left in flight on the harness's first stream (smh_gather with other_stream = 1 then runs beside them).
extern "C" int smh_fill(void* hv, int n_desc, const uint64_t* sig_off, const uint64_t* par_off, const uint64_t* seg_off, const uint32_t* T,
                        const uint32_t* N, const uint32_t* read, int n_state, const int32_t* status, uint64_t n_sig, const double* sig,
                        uint64_t n_seg, const uint32_t* segrow, uint64_t n_par, const uint32_t* sites, uint32_t read_lo, uint32_t read_hi,
                        int runs, int sync) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || n_desc < 1 || n_state < 1 || n_sig < 1 || n_seg < 1 || n_par < 1 || runs < 1 || runs > 4) return -1;
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
  TRY(hipStreamSynchronize(h->s));
  if (int rc = free_batch(h)) return rc;
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
  void *d_descs = nullptr, *d_st = nullptr, *d_sig = nullptr, *d_segrow = nullptr, *d_sites = nullptr;
  if (int rc = upload(h, &d_descs, descs.data(), descs.size() * sizeof(ReadDesc))) return rc;
  if (int rc = upload(h, &d_st, st.data(), st.size() * sizeof(ReadState))) return rc;
  if (int rc = upload(h, &d_sig, sig, n_sig * 8)) return rc;
  if (int rc = upload(h, &d_segrow, segrow, n_seg * 4)) return rc;
  if (int rc = upload(h, &d_sites, sites, n_par * 4)) return rc;
  TRY(hipStreamSynchronize(h->s));  // (descs and st are host vectors of this call)
  dynk::SiteSummary ss{static_cast<const double*>(d_sig), static_cast<const uint32_t*>(d_sites), h->acc, h->totals(), h->num_sites, read_lo, read_hi};
  if (h->bins) {
    ss.hist = h->hist;
    ss.bins = h->bins;
    ss.hist_lo = h->lo;
    ss.inv_w = h->inv_w;
  }
  ss.map_keys = h->keys;
  ss.capacity = h->capacity;
  ss.map_stats = h->stats();
  for (int r = 0; r < runs; ++r)
    dynk::launch_site_summary_kernels(static_cast<const ReadDesc*>(d_descs), n_desc, max_N, static_cast<const ReadState*>(d_st),
                                      static_cast<const uint32_t*>(d_segrow), ss, h->s);
  TRY(hipGetLastError());
  if (sync) TRY(hipStreamSynchronize(h->s));
  return 0;
}

// k_site_gather over the ids [lo, lo + count): out_acc [count][7] (nullptr: the counters alone), out_hist [count][width]
// (nullptr: the table alone). other_stream: on the second stream, beside whatever smh_fill(sync = 0) left in flight; both
// streams are waited for before it returns.
extern "C" int smh_gather(void* hv, uint32_t lo, uint32_t count, uint64_t* out_acc, uint32_t* out_hist, int other_stream) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || count < 1 || (uint64_t)lo + count > h->num_sites || (!out_acc && !out_hist) || (out_hist && !h->bins)) return -1;
  hipStream_t s = other_stream ? h->s2 : h->s;
  void *d_acc = nullptr, *d_hist = nullptr;
  const size_t b_acc = (size_t)count * dynk::SS_FIELDS * 8, b_hist = (size_t)count * h->width * 4;
  int rc = 0;
  auto run = [&]() -> int {
    if (out_acc) TRY(hipMalloc(&d_acc, b_acc));
    if (out_hist) TRY(hipMalloc(&d_hist, b_hist));
    if (out_acc) TRY(hipMemsetAsync(d_acc, 0xA5, b_acc, s));  // (an absent id must come back as zeros the kernel wrote)
    if (out_hist) TRY(hipMemsetAsync(d_hist, 0xA5, b_hist, s));
    dynk::SiteGather sg{};
    sg.keys = h->keys;
    sg.capacity = h->capacity;
    sg.acc = h->acc;
    sg.hist = out_hist ? h->hist : nullptr;
    sg.width = h->width;
    sg.lo = lo;
    sg.count = count;
    sg.out_acc = static_cast<unsigned long long*>(d_acc);
    sg.out_hist = static_cast<unsigned int*>(d_hist);
    dynk::launch_site_gather_kernel(sg, s);
    TRY(hipGetLastError());
    if (out_acc) TRY(hipMemcpyAsync(out_acc, d_acc, b_acc, hipMemcpyDeviceToHost, s));
    if (out_hist) TRY(hipMemcpyAsync(out_hist, d_hist, b_hist, hipMemcpyDeviceToHost, s));
    TRY(hipStreamSynchronize(s));
    TRY(hipStreamSynchronize(h->s));
    return 0;
  };
  rc = run();
  for (void* p : {d_acc, d_hist})
    if (p) {
      const hipError_t e = hipFree(p);
      if (e != hipSuccess && !rc) rc = (int)e;
    }
  return rc;
}

// k_site_scatter_add of a staged window: cols [count][7], counters [count][width] or nullptr, totals_in [5] or nullptr
extern "C" int smh_scatter(void* hv, uint32_t lo, uint32_t count, const uint64_t* cols, const uint32_t* counters, const uint64_t* totals_in) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || count < 1 || (uint64_t)lo + count > h->num_sites || !cols || (counters && !h->bins)) return -1;
  void *d_cols = nullptr, *d_cnt = nullptr;
  const size_t b_cols = (size_t)count * dynk::SS_FIELDS * 8, b_cnt = (size_t)count * h->width * 4;
  auto run = [&]() -> int {
    TRY(hipMalloc(&d_cols, b_cols));
    TRY(hipMemcpyAsync(d_cols, cols, b_cols, hipMemcpyHostToDevice, h->s));
    if (counters) {
      TRY(hipMalloc(&d_cnt, b_cnt));
      TRY(hipMemcpyAsync(d_cnt, counters, b_cnt, hipMemcpyHostToDevice, h->s));
    }
    dynk::SiteScatter sc{};
    sc.keys = h->keys;
    sc.capacity = h->capacity;
    sc.stats = h->stats();
    sc.acc = h->acc;
    sc.totals = h->totals();
    sc.hist = counters ? h->hist : nullptr;
    sc.cols = static_cast<const unsigned long long*>(d_cols);
    sc.counters = static_cast<const unsigned int*>(d_cnt);
    sc.width = h->width;
    sc.lo = lo;
    sc.count = count;
    sc.add_totals = totals_in ? 1 : 0;
    for (int f = 0; f < dynk::SS_TOTALS; ++f) sc.totals_in[f] = totals_in ? totals_in[f] : 0ull;
    dynk::launch_site_scatter_add_kernel(sc, h->s);
    TRY(hipGetLastError());
    TRY(hipStreamSynchronize(h->s));
    return 0;
  };
  int rc = run();
  for (void* p : {d_cols, d_cnt})
    if (p) {
      const hipError_t e = hipFree(p);
      if (e != hipSuccess && !rc) rc = (int)e;
    }
  return rc;
}

// k_site_map_windows: bitmap of n_words uint32, which must hold bit (num_sites - 1) >> shift
extern "C" int smh_windows(void* hv, int shift, uint32_t* bitmap, uint64_t n_words) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || shift < 0 || shift > 31 || !bitmap || n_words < ((((uint64_t)h->num_sites - 1) >> shift) + 32) / 32) return -1;
  void* d = nullptr;
  auto run = [&]() -> int {
    TRY(hipMalloc(&d, n_words * 4));
    TRY(hipMemsetAsync(d, 0, n_words * 4, h->s));
    dynk::launch_site_map_windows_kernel(dynk::SiteWindows{h->keys, h->capacity, shift, static_cast<unsigned int*>(d)}, h->s);
    TRY(hipGetLastError());
    TRY(hipMemcpyAsync(bitmap, d, n_words * 4, hipMemcpyDeviceToHost, h->s));
    TRY(hipStreamSynchronize(h->s));
    return 0;
  };
  int rc = run();
  if (d) {
    const hipError_t e = hipFree(d);
    if (e != hipSuccess && !rc) rc = (int)e;
  }
  return rc;
}

// the map as the device holds it: keys [capacity], acc [7 capacity + 5 + 3] (cells, totals, statistics), hist [capacity][width]
extern "C" int smh_raw(void* hv, uint32_t* keys, uint64_t* acc, uint32_t* hist) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || !keys || !acc || (hist && !h->bins)) return -1;
  TRY(hipStreamSynchronize(h->s));
  TRY(hipMemcpy(keys, h->keys, (size_t)h->capacity * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(acc, h->acc, h->acc_words() * 8, hipMemcpyDeviceToHost));
  if (hist) TRY(hipMemcpy(hist, h->hist, (size_t)h->capacity * h->width * 4, hipMemcpyDeviceToHost));
  return 0;
}
