// site_pack.hip -- test-only translation unit (tests/test_gpu_site_pack.py, tests/test_site_pack_host.py): the pack and the merge
// of the per-site table (site_pack_kernels.hpp: k_site_pack_count, k_site_pack_scan, k_site_pack_write, k_site_merge) on tables
// the HOST hands in, dense or behind a map. Every integer is compared with a Python-int restatement (tests/site_pack_cases.py).
// The constants the shapes of the tests depend on are exported, as sm_home and SM_PROBE_MAX are by site_map.hip.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes. Every call returns 0, a hipError_t, or -1 for an argument that would index outside what was handed in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "site_map_kernels.hpp"
#include "site_pack_kernels.hpp"

namespace {
struct Harness {
  uint32_t num_sites = 0, capacity = 0, rows = 0, width = 0;  // capacity == 0: dense, rows = num_sites
  uint32_t* keys = nullptr;
  unsigned long long* acc = nullptr;  // [7 rows + 5 + 3]
  unsigned int* hist = nullptr;       // [rows][width]; nullptr: width == 0
  hipStream_t s = nullptr;
  size_t acc_words() const { return (size_t)rows * dynk::SS_FIELDS + dynk::SS_TOTALS + dynk::SM_STATS; }
  unsigned long long* totals() const { return acc + (size_t)rows * dynk::SS_FIELDS; }
  unsigned long long* stats() const { return totals() + dynk::SS_TOTALS; }
};

#define TRY(x)                             \
  do {                                     \
    const hipError_t e_ = (x);             \
    if (e_ != hipSuccess) return (int)e_;  \
  } while (0)

int free_all(std::initializer_list<void*> ps, int rc) {
  for (void* p : ps)
    if (p) {
      const hipError_t e = hipFree(p);
      if (e != hipSuccess && !rc) rc = (int)e;
    }
  return rc;
}
}  // namespace

extern "C" uint32_t sph_home(uint32_t id, uint32_t capacity) { return dynk::sm_home(id, capacity); }
extern "C" void sph_home_many(const uint32_t* ids, uint64_t n, uint32_t capacity, uint32_t* out) {
  for (uint64_t i = 0; i < n; ++i) out[i] = dynk::sm_home(ids[i], capacity);
}
extern "C" uint32_t sph_probe_max() { return dynk::SM_PROBE_MAX; }
extern "C" uint32_t sph_chunk_rows() { return dynk::SPK_CHUNK_ROWS; }
extern "C" uint32_t sph_scan_tile_rows() { return dynk::SPK_SCAN_TILE_ROWS; }
extern "C" uint32_t sph_lanes() { return dynk::SMK_LANES; }

// a zeroed table over the ids below num_sites: dense (capacity == 0, num_sites rows) or behind an empty map of `capacity` rows;
// bins > 0: bins + 2 + 16 counters per row
extern "C" int sph_create(uint32_t num_sites, uint32_t capacity, uint32_t bins, void** out) {
  if (!out || num_sites < 1 || num_sites == 0xFFFFFFFFu || capacity == 0xFFFFFFFFu || bins > (uint32_t)dynk::SH_BINS_MAX) return -1;
  Harness* h = new Harness();
  *out = h;
  h->num_sites = num_sites;
  h->capacity = capacity;
  h->rows = capacity ? capacity : num_sites;
  h->width = bins ? bins + 2u + (uint32_t)dynk::SH_DWELL_BINS : 0u;
  TRY(hipStreamCreateWithFlags(&h->s, hipStreamNonBlocking));
  if (capacity) TRY(hipMalloc(reinterpret_cast<void**>(&h->keys), (size_t)capacity * 4));
  TRY(hipMalloc(reinterpret_cast<void**>(&h->acc), h->acc_words() * 8));
  if (bins) TRY(hipMalloc(reinterpret_cast<void**>(&h->hist), (size_t)h->rows * h->width * 4));
  if (capacity) TRY(hipMemsetAsync(h->keys, 0xFF, (size_t)capacity * 4, h->s));
  TRY(hipMemsetAsync(h->acc, 0, h->acc_words() * 8, h->s));
  if (bins) TRY(hipMemsetAsync(h->hist, 0, (size_t)h->rows * h->width * 4, h->s));
  TRY(hipStreamSynchronize(h->s));
  return 0;
}

extern "C" int sph_destroy(void* hv) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h) return -1;
  int rc = free_all({h->keys, h->acc, h->hist}, 0);
  if (h->s) {
    const hipError_t e = hipStreamDestroy(h->s);
    if (e != hipSuccess && !rc) rc = (int)e;
  }
  delete h;
  return rc;
}

// the table as the test wants it: keys [capacity] (a sparse table; nullptr leaves them), cells [rows][7], hist [rows][width]
extern "C" int sph_set(void* hv, const uint32_t* keys, const uint64_t* cells, const uint32_t* hist) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || !cells || (keys && !h->capacity) || (hist && !h->width) || (!hist && h->width)) return -1;
  if (keys)
    for (uint32_t b = 0; b < h->capacity; ++b)
      if (keys[b] != dynk::SM_EMPTY && keys[b] >= h->num_sites) return -1;
  if (keys) TRY(hipMemcpyAsync(h->keys, keys, (size_t)h->capacity * 4, hipMemcpyHostToDevice, h->s));
  TRY(hipMemcpyAsync(h->acc, cells, (size_t)h->rows * dynk::SS_FIELDS * 8, hipMemcpyHostToDevice, h->s));
  if (hist) TRY(hipMemcpyAsync(h->hist, hist, (size_t)h->rows * h->width * 4, hipMemcpyHostToDevice, h->s));
  TRY(hipStreamSynchronize(h->s));
  return 0;
}

// the three passes over the rows [row_lo, row_lo + count): *total live rows; the first min(*total, cap) records into site [cap],
// cells [cap][7], counters [cap][width]. The records' device arrays hold exactly *total entries, filled with 0xA5 beforehand
// and with a guard entry behind them that must come back untouched (-2 otherwise).
extern "C" int sph_pack(void* hv, uint32_t row_lo, uint32_t count, uint32_t site_lo, uint32_t site_hi, uint64_t cap, uint32_t* site,
                        uint64_t* cells, uint32_t* counters, uint64_t* total) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || !total || count > (1u << 20) || (uint64_t)row_lo + count > h->rows || site_lo > site_hi || site_hi > h->num_sites) return -1;
  if (cap && (!site || !cells || (h->width && !counters))) return -1;
  *total = 0;
  if (count == 0) return 0;
  const size_t chunks = ((size_t)count + dynk::SPK_CHUNK_ROWS - 1) / dynk::SPK_CHUNK_ROWS;
  void *d_scan = nullptr, *d_site = nullptr, *d_cells = nullptr, *d_cnt = nullptr;
  const size_t F = dynk::SS_FIELDS, W = h->width;
  auto run = [&]() -> int {
    TRY(hipMalloc(&d_scan, 8 + chunks * 12));
    TRY(hipMemsetAsync(d_scan, 0xA5, 8 + chunks * 12, h->s));
    dynk::SitePack sp{};
    sp.keys = h->keys;
    sp.acc = h->acc;
    sp.hist = h->hist;
    sp.width = h->width;
    sp.row_lo = row_lo;
    sp.count = count;
    sp.site_lo = site_lo;
    sp.site_hi = site_hi;
    sp.total = static_cast<unsigned long long*>(d_scan);
    sp.mask = sp.total + 1;
    sp.offset = reinterpret_cast<uint32_t*>(sp.mask + chunks);
    dynk::launch_site_pack_kernels(sp, h->s);
    TRY(hipGetLastError());
    unsigned long long n = 0;
    TRY(hipMemcpyAsync(&n, sp.total, 8, hipMemcpyDeviceToHost, h->s));
    TRY(hipStreamSynchronize(h->s));
    *total = n;
    if (n > count) return -2;
    if (n == 0) return 0;
    TRY(hipMalloc(&d_site, (n + 1) * 4));
    TRY(hipMalloc(&d_cells, (n + 1) * F * 8));
    TRY(hipMemsetAsync(d_site, 0xA5, (n + 1) * 4, h->s));
    TRY(hipMemsetAsync(d_cells, 0xA5, (n + 1) * F * 8, h->s));
    if (W) {
      TRY(hipMalloc(&d_cnt, (n + 1) * W * 4));
      TRY(hipMemsetAsync(d_cnt, 0xA5, (n + 1) * W * 4, h->s));
    }
    sp.cap = n;
    sp.out_site = static_cast<uint32_t*>(d_site);
    sp.out_cells = static_cast<unsigned long long*>(d_cells);
    sp.out_hist = static_cast<unsigned int*>(d_cnt);
    dynk::launch_site_pack_write_kernel(sp, h->s);
    TRY(hipGetLastError());
    const size_t m = (size_t)std::min<uint64_t>(n, cap);
    uint32_t g_site = 0;
    std::vector<unsigned long long> g_cells(F);
    std::vector<unsigned int> g_cnt(W);
    TRY(hipMemcpyAsync(&g_site, sp.out_site + n, 4, hipMemcpyDeviceToHost, h->s));
    TRY(hipMemcpyAsync(g_cells.data(), sp.out_cells + n * F, F * 8, hipMemcpyDeviceToHost, h->s));
    if (W) TRY(hipMemcpyAsync(g_cnt.data(), sp.out_hist + n * W, W * 4, hipMemcpyDeviceToHost, h->s));
    if (m) {
      TRY(hipMemcpyAsync(site, d_site, m * 4, hipMemcpyDeviceToHost, h->s));
      TRY(hipMemcpyAsync(cells, d_cells, m * F * 8, hipMemcpyDeviceToHost, h->s));
      if (W) TRY(hipMemcpyAsync(counters, d_cnt, m * W * 4, hipMemcpyDeviceToHost, h->s));
    }
    TRY(hipStreamSynchronize(h->s));
    if (g_site != 0xA5A5A5A5u) return -2;
    for (unsigned long long v : g_cells)
      if (v != 0xA5A5A5A5A5A5A5A5ull) return -2;
    for (unsigned int v : g_cnt)
      if (v != 0xA5A5A5A5u) return -2;
    return 0;
  };
  const int rc = run();
  return free_all({d_scan, d_site, d_cells, d_cnt}, rc);
}

// k_site_merge of `count` records in ONE launch: site [count], cells [count][7], counters [count][width] or nullptr (the table
// alone), totals_in [5] or nullptr. Every site[i] + offset must lie below num_sites.
extern "C" int sph_merge(void* hv, uint32_t count, const uint32_t* site, uint64_t offset, const uint64_t* cells, const uint32_t* counters,
                         const uint64_t* totals_in) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || count < 1 || !site || !cells || (counters && !h->width)) return -1;
  for (uint32_t i = 0; i < count; ++i)
    if (offset >= h->num_sites || site[i] >= h->num_sites - offset) return -1;
  void *d_site = nullptr, *d_cells = nullptr, *d_cnt = nullptr;
  const size_t F = dynk::SS_FIELDS, W = h->width;
  auto run = [&]() -> int {
    TRY(hipMalloc(&d_site, (size_t)count * 4));
    TRY(hipMalloc(&d_cells, (size_t)count * F * 8));
    TRY(hipMemcpyAsync(d_site, site, (size_t)count * 4, hipMemcpyHostToDevice, h->s));
    TRY(hipMemcpyAsync(d_cells, cells, (size_t)count * F * 8, hipMemcpyHostToDevice, h->s));
    if (counters) {
      TRY(hipMalloc(&d_cnt, (size_t)count * W * 4));
      TRY(hipMemcpyAsync(d_cnt, counters, (size_t)count * W * 4, hipMemcpyHostToDevice, h->s));
    }
    dynk::SiteMerge sm{};
    sm.keys = h->keys;
    sm.capacity = h->capacity;
    sm.stats = h->stats();
    sm.acc = h->acc;
    sm.totals = h->totals();
    sm.hist = counters ? h->hist : nullptr;
    sm.site = static_cast<const uint32_t*>(d_site);
    sm.cells = static_cast<const unsigned long long*>(d_cells);
    sm.counters = static_cast<const unsigned int*>(d_cnt);
    sm.width = h->width;
    sm.count = count;
    sm.offset = offset;
    sm.num_sites = h->num_sites;
    sm.add_totals = totals_in ? 1 : 0;
    for (int f = 0; f < dynk::SS_TOTALS; ++f) sm.totals_in[f] = totals_in ? totals_in[f] : 0ull;
    dynk::launch_site_merge_kernel(sm, h->s);
    TRY(hipGetLastError());
    TRY(hipStreamSynchronize(h->s));
    return 0;
  };
  const int rc = run();
  return free_all({d_site, d_cells, d_cnt}, rc);
}

// the ids [lo, lo + count) as a dense window: k_site_gather through the map of a sparse table, the rows themselves of a dense one
extern "C" int sph_window(void* hv, uint32_t lo, uint32_t count, uint64_t* out_acc, uint32_t* out_hist) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || count < 1 || (uint64_t)lo + count > h->num_sites || !out_acc || (out_hist && !h->width)) return -1;
  const size_t b_acc = (size_t)count * dynk::SS_FIELDS * 8, b_hist = (size_t)count * h->width * 4;
  if (!h->capacity) {
    TRY(hipStreamSynchronize(h->s));
    TRY(hipMemcpy(out_acc, h->acc + (size_t)lo * dynk::SS_FIELDS, b_acc, hipMemcpyDeviceToHost));
    if (out_hist) TRY(hipMemcpy(out_hist, h->hist + (size_t)lo * h->width, b_hist, hipMemcpyDeviceToHost));
    return 0;
  }
  void *d_acc = nullptr, *d_hist = nullptr;
  auto run = [&]() -> int {
    TRY(hipMalloc(&d_acc, b_acc));
    if (out_hist) TRY(hipMalloc(&d_hist, b_hist));
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
    dynk::launch_site_gather_kernel(sg, h->s);
    TRY(hipGetLastError());
    TRY(hipMemcpyAsync(out_acc, d_acc, b_acc, hipMemcpyDeviceToHost, h->s));
    if (out_hist) TRY(hipMemcpyAsync(out_hist, d_hist, b_hist, hipMemcpyDeviceToHost, h->s));
    TRY(hipStreamSynchronize(h->s));
    return 0;
  };
  const int rc = run();
  return free_all({d_acc, d_hist}, rc);
}

// the table as the device holds it: keys [capacity] (sparse), acc [7 rows + 5 + 3] (cells, totals, statistics), hist [rows][width]
extern "C" int sph_raw(void* hv, uint32_t* keys, uint64_t* acc, uint32_t* hist) {
  Harness* h = static_cast<Harness*>(hv);
  if (!h || !acc || (keys && !h->capacity) || (hist && !h->width)) return -1;
  TRY(hipStreamSynchronize(h->s));
  if (keys) TRY(hipMemcpy(keys, h->keys, (size_t)h->capacity * 4, hipMemcpyDeviceToHost));
  TRY(hipMemcpy(acc, h->acc, h->acc_words() * 8, hipMemcpyDeviceToHost));
  if (hist) TRY(hipMemcpy(hist, h->hist, (size_t)h->rows * h->width * 4, hipMemcpyDeviceToHost));
  return 0;
}
