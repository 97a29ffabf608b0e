// site_table.cpp -- the per-site table of a handle (dyneng::SiteTable, engine.hpp: dyn_aligner::site) behind the C ABI: its two
// setters, the staged ids, the map's getters and the window calls that read or add to a range of sites. The kernels:
// site_summary_kernels.hpp (the table, its histograms, the quantiles), site_compare_kernels.hpp, site_mixture_kernels.hpp,
// site_map_kernels.hpp (the sparse table), site_pack_kernels.hpp (the table by content); what a JOB adds to the table is launched with the job (launch.cpp).
//
// A window call holds the handle's lock throughout and runs every copy and kernel on s_get. It walks its range in windows of
// 2^20 sites (Windows), points its kernel's argument struct at each (table_window / hist_window: the table itself, or the gathered
// scratch of a sparse one), launches, copies the window's output into a host vector and unpacks that into the caller's columns
// at the window's offset.
#include "engine_internal.hpp"
#include "dp_math_strict.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

using namespace dyneng;

namespace {

int fail(dyn_aligner* a, const char* who, const std::string& msg, int rc = DYN_ERR_INVALID_ARGUMENT) {
  std::lock_guard<std::mutex> lk(a->err_mu);
  a->last_error = std::string(who) + ": " + msg;
  return rc;
}

const char* const NO_TABLE = "dyn_aligner_set_site_summary(a, num_sites > 0) was never called on this handle";

// ---- what a call needs before it touches the table ---------------------------------------------------------------------------
// every kernel that adds to the table runs on the compute stream (one launch per batch) or on the copy-out stream (tickets of a
// resident session): the table of the jobs that have completed is behind both
int site_summary_quiet(dyn_aligner* a, const char* who) {
  if (int rc = need_device(a)) return rc;
  if (!a->site.table.p) return fail(a, who, NO_TABLE);
  HIP_TRY(a, hipStreamSynchronize(a->stream));
  HIP_TRY(a, hipStreamSynchronize(a->s_out));
  return DYN_OK;
}

bool in_table(const dyn_aligner* a, uint64_t lo, uint64_t hi) { return lo <= hi && hi <= a->site.num_sites; }
std::string no_range(const dyn_aligner* a, uint64_t lo, uint64_t hi) {
  return "[" + std::to_string(lo) + ", " + std::to_string(hi) + ") is not a range of the table's " + std::to_string(a->site.num_sites) + " sites";
}
// the second window of a pair call: n sites from other_lo
bool other_in_table(const dyn_aligner* a, uint64_t other_lo, uint64_t n) { return other_lo <= a->site.num_sites && n <= a->site.num_sites - other_lo; }
std::string no_other_window(const dyn_aligner* a, uint64_t other_lo, uint64_t n) {
  return "the other window [" + std::to_string(other_lo) + ", " + std::to_string(other_lo) + " + " + std::to_string(n) + ") does not end inside the table's " +
         std::to_string(a->site.num_sites) + " sites";
}

// ... and [lo, hi) a range of the table
int site_range_quiet(dyn_aligner* a, const char* who, uint64_t lo, uint64_t hi) {
  if (int rc = site_summary_quiet(a, who)) return rc;
  return in_table(a, lo, hi) ? DYN_OK : fail(a, who, no_range(a, lo, hi));
}

// ... and, before the range is looked at, histograms to read
int site_histogram_quiet(dyn_aligner* a, const char* who, uint64_t lo, uint64_t hi) {
  if (int rc = site_summary_quiet(a, who)) return rc;
  if (!a->site.has_hist()) return fail(a, who, "dyn_aligner_set_site_histogram(a, bins > 0, lo, hi) was never called on this handle");
  return in_table(a, lo, hi) ? DYN_OK : fail(a, who, no_range(a, lo, hi));
}

// the conditions of the calls that read the map: a sparse table, completed jobs
int site_map_quiet(dyn_aligner* a, const char* who) {
  if (int rc = site_summary_quiet(a, who)) return rc;
  if (!a->site.sparse() || !a->site.keys.p)
    return fail(a, who, "the per-site table of this handle is dense (dyn_aligner_set_site_summary_sparse sets a sparse one)");
  return DYN_OK;
}

// ---- the setters' two steps ------------------------------------------------------------------------------------------------------
// Before a buffer that jobs add to is replaced. The switch goes off BEFORE the lock is dropped: a ticket another thread submits
// while this call drains takes no part, so none can add to what is about to be freed. The jobs in flight hold the old address
// (snapshot at their submission) -- they finish first; then no resident wave may be waiting for tickets (hipFree waits for the
// whole device: under an open session until its idle watchdog), and both streams that add have passed. Returns under the lock.
int retire_and_wait(dyn_aligner* a, std::unique_lock<std::mutex>& lk, bool JobOptions::*flag) {
  a->opt.*flag = false;
  Pipeline* pipe = a->pipe.get();
  lk.unlock();
  if (pipe) pipe->drain();
  lk.lock();
  if (int rc = session_quiesce(a)) return rc;
  HIP_TRY(a, hipStreamSynchronize(a->stream));
  HIP_TRY(a, hipStreamSynchronize(a->s_out));
  a->opt.*flag = false;
  return DYN_OK;
}

// The buffers of one setter, allocated together and filled: refused where their sum does not fit what the memory budget leaves
// (`what` `fits` ...: "the table of 5 sites (315 bytes)" "does not fit"), all released where one cannot be had.
struct Filled {
  DevBuf* d;
  uint64_t bytes;  // 0: not wanted
  int fill;        // the byte it starts from
};
int alloc_zeroed(dyn_aligner* a, const char* who, const std::string& what, const char* fits, std::initializer_list<Filled> bufs) {
  uint64_t bytes = 0;
  for (const Filled& b : bufs) bytes += b.bytes;
  if (a->mem_budget && bytes > mem_budget_left(a))
    return fail(a, who, what + " " + fits + " dyn_aligner_set_mem_budget's " + std::to_string(a->mem_budget) + " bytes", DYN_ERR_OUT_OF_MEMORY);
  hipError_t e = hipSuccess;
  for (const Filled& b : bufs)
    if (e == hipSuccess && b.bytes) e = b.d->ensure(b.bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    for (const Filled& b : bufs) b.d->release();
    return fail(a, who, "no device memory for " + what + ": " + hipGetErrorString(e), e == hipErrorOutOfMemory ? DYN_ERR_OUT_OF_MEMORY : DYN_ERR_DEVICE);
  }
  for (const Filled& b : bufs)
    if (b.bytes) HIP_TRY(a, hipMemsetAsync(b.d->p, b.fill, b.bytes, a->s_get));
  HIP_TRY(a, hipStreamSynchronize(a->s_get));
  return DYN_OK;
}

// both setters of the table: capacity == 0 is the dense table of num_sites rows, capacity > 0 the sparse one of capacity rows
// behind a map (site_map.hpp) whose ids stay below num_sites
int set_site_table(dyn_aligner* a, uint64_t num_sites, uint64_t capacity, const char* who) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const bool sparse = capacity > 0;
  if (a->ntk) return fail(a, who, "modes ntk / resquiggle have no align(calc_probabilities = 1) job to summarise");
  if (num_sites >= (uint64_t)DYN_SITE_NONE) return fail(a, who, "num_sites " + std::to_string(num_sites) + " is not below DYN_SITE_NONE (4294967295)");
  if (capacity >= (uint64_t)DYN_SITE_NONE) return fail(a, who, "capacity " + std::to_string(capacity) + " is not below 4294967295");
  std::unique_lock<std::mutex> lk(a->mu);
  SiteTable& t = a->site;
  if (int rc = need_device(a)) return rc;
  if (num_sites == 0) {  // off: the table stays for the fetch
    a->opt.site_summary = false;
    return DYN_OK;
  }
  if (num_sites == t.num_sites && capacity == t.capacity && t.table.p) {
    a->opt.site_summary = true;
    return DYN_OK;
  }
  // another size or mode
  if (int rc = retire_and_wait(a, lk, &JobOptions::site_summary)) return rc;
  // the histograms were the old table's: released and off with it, the caller sets them again (dyn_aligner_set_site_histogram)
  t.release_table();
  a->opt.site_histogram = false;
  const uint64_t rows = sparse ? capacity : num_sites;
  const uint64_t key_bytes = sparse ? capacity * sizeof(uint32_t) : 0;
  const uint64_t table_bytes = SiteTable::words(rows, sparse) * sizeof(uint64_t);
  const std::string size = " (" + std::to_string(table_bytes + key_bytes) + " bytes)";
  const std::string what = sparse ? "the sparse table of " + std::to_string(capacity) + " rows" + size : "the table of " + std::to_string(num_sites) + " sites" + size;
  if (int rc = alloc_zeroed(a, who, what, "does not fit", {{&t.table, table_bytes, 0}, {&t.keys, key_bytes, 0xFF}})) return rc;
  t.num_sites = num_sites;
  t.capacity = capacity;
  a->opt.site_summary = true;
  return DYN_OK;
}

// ---- the windows of a call ---------------------------------------------------------------------------------------------------------
constexpr uint64_t STEP = 1ull << 20;  // sites per window: 56 MB of cells at a time

// the n sites from lo in windows of at most STEP: `for (auto [s0, cnt, o] : Windows(lo, n))` sees the window's first site, its
// sites and its offset s0 - lo in the caller's columns. most: the largest window, which sizes the staging of the whole call
struct Windows {
  uint64_t lo, n, most;
  Windows(uint64_t lo_, uint64_t n_) : lo(lo_), n(n_), most(std::min(STEP, n_)) {}
  struct Window {
    uint64_t s0, cnt, o;
  };
  struct Iter {
    const Windows* w;
    uint64_t o;
    Window operator*() const { return {w->lo + o, std::min(STEP, w->n - o), o}; }
    void operator++() { o += STEP; }
    bool operator!=(const Iter&) const { return o < w->n; }
  };
  Iter begin() const { return {this, 0}; }
  Iter end() const { return {this, n}; }
};

// A window of a sparse table as the dense calls see one. The ids [s0, s0 + cnt) are gathered on s_get into slot `slot` of the
// `slots` (1, or 2 where a call reads two windows at once) of the scratch, each sized for `most` sites of what the call asks for
// -- every gather of one call asks for the same: the cells [cnt][7] u64, or (hist) the counters [cnt][bins + 2 + 16] uint32. The
// scratch grows on first use and counts against the memory budget (SiteTable::held_bytes). The window kernels and copies behind
// the gather on s_get read the scratch.
template <class T>
int gather_window(dyn_aligner* a, uint64_t s0, uint64_t cnt, uint64_t most, int slot, int slots, bool hist, const T** out) {
  SiteTable& t = a->site;
  const uint64_t row_bytes = hist ? t.hist_width() * sizeof(uint32_t) : (uint64_t)dynk::SS_FIELDS * sizeof(uint64_t);
  const uint64_t slot_bytes = (most * row_bytes + 7) / 8 * 8;  // (rounded up: every slot starts 8-byte aligned)
  HIP_TRY(a, t.gather.ensure((uint64_t)slots * slot_bytes));
  char* base = t.gather.as<char>() + (uint64_t)slot * slot_bytes;
  dynk::SiteGather sg{};
  sg.keys = t.keys.as<uint32_t>();
  sg.capacity = (uint32_t)t.capacity;
  sg.acc = t.table.as<unsigned long long>();
  sg.lo = (uint32_t)s0;
  sg.count = (uint32_t)cnt;
  if (hist) {
    sg.hist = t.hist.as<unsigned int>();
    sg.width = (uint32_t)t.hist_width();
    sg.out_hist = reinterpret_cast<unsigned int*>(base);
  } else {
    sg.out_acc = reinterpret_cast<unsigned long long*>(base);
  }
  dynk::launch_site_gather(sg, a->s_get);
  HIP_TRY(a, hipGetLastError());
  *out = reinterpret_cast<const T*>(base);
  return DYN_OK;
}

// where a window call reads the cells / the counters of the sites [s0, s0 + cnt): in the table itself, or in the gathered slot
int table_window(dyn_aligner* a, uint64_t s0, uint64_t cnt, uint64_t most, int slot, int slots, const uint64_t** cells) {
  if (a->site.sparse()) return gather_window(a, s0, cnt, most, slot, slots, false, cells);
  *cells = a->site.table.as<uint64_t>() + (uint64_t)dynk::SS_FIELDS * s0;
  return DYN_OK;
}
int hist_window(dyn_aligner* a, uint64_t s0, uint64_t cnt, uint64_t most, int slot, int slots, const unsigned int** counters) {
  if (a->site.sparse()) return gather_window(a, s0, cnt, most, slot, slots, true, counters);
  *counters = a->site.hist.as<unsigned int>() + a->site.hist_width() * s0;
  return DYN_OK;
}

}  // namespace

extern "C" {

// ---- the table and its map (site_summary_kernels.hpp, site_map.hpp) ----------------------------------------------------------------
int dyn_aligner_set_site_summary(dyn_aligner* a, uint64_t num_sites) { return set_site_table(a, num_sites, 0, "dyn_aligner_set_site_summary"); }

int dyn_aligner_set_site_summary_sparse(dyn_aligner* a, uint64_t num_sites, uint64_t capacity) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_set_site_summary_sparse";
  if (num_sites && !capacity) return fail(a, who, "capacity 0 is no table (dyn_aligner_set_site_summary sets a dense one)");
  return set_site_table(a, num_sites, num_sites ? capacity : 0, who);
}

int dyn_aligner_stage_site_ids(dyn_aligner* a, const uint32_t* site_ids, uint64_t count) {
  if (!a || (count && !site_ids)) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  a->site.staged_ids = site_ids;
  a->site.staged_count = count;
  a->site.staged = true;
  return DYN_OK;
}

int dyn_aligner_site_map_stats(dyn_aligner* a, uint64_t out[4]) {
  if (!a || !out) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_map_quiet(a, "dyn_aligner_site_map_stats")) return rc;
  out[0] = a->site.capacity;
  HIP_TRY(a, copy_out(a, out + 1, a->site.totals() + dynk::SS_TOTALS, (uint64_t)dynk::SM_STATS * sizeof(uint64_t)));
  return DYN_OK;
}

int dyn_aligner_site_map_keys(dyn_aligner* a, uint64_t bucket_lo, uint64_t bucket_hi, uint32_t* keys) {
  if (!a || (bucket_lo < bucket_hi && !keys)) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_map_keys";
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_map_quiet(a, who)) return rc;
  if (bucket_lo > bucket_hi || bucket_hi > a->site.capacity)
    return fail(a, who, "[" + std::to_string(bucket_lo) + ", " + std::to_string(bucket_hi) + ") is not a range of the map's " + std::to_string(a->site.capacity) + " buckets");
  if (bucket_lo == bucket_hi) return DYN_OK;
  HIP_TRY(a, copy_out(a, keys, a->site.keys.as<uint32_t>() + bucket_lo, (bucket_hi - bucket_lo) * sizeof(uint32_t)));
  return DYN_OK;
}

int dyn_aligner_site_map_windows(dyn_aligner* a, int shift, uint64_t* windows, uint64_t cap, uint64_t* count) {
  if (!a || !count || (cap && !windows)) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_map_windows";
  if (shift < 0 || shift > 31) return fail(a, who, "shift " + std::to_string(shift) + " is not 0 .. 31");
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_map_quiet(a, who)) return rc;
  SiteTable& t = a->site;
  const uint64_t n_win = ((t.num_sites - 1) >> shift) + 1;  // (a table has num_sites >= 1)
  if (n_win > (1ull << 22))
    return fail(a, who, "shift " + std::to_string(shift) + " cuts the " + std::to_string(t.num_sites) + " ids into " + std::to_string(n_win) + " windows, more than 4194304");
  const uint64_t words = (n_win + 31) / 32;
  DevBuf& bitmap = t.window_bitmap();
  HIP_TRY(a, bitmap.ensure(words * sizeof(uint32_t)));
  HIP_TRY(a, hipMemsetAsync(bitmap.p, 0, words * sizeof(uint32_t), a->s_get));
  dynk::SiteWindows sw{t.keys.as<uint32_t>(), (uint32_t)t.capacity, shift, bitmap.as<unsigned int>()};
  dynk::launch_site_map_windows(sw, a->s_get);
  HIP_TRY(a, hipGetLastError());
  std::vector<uint32_t> h(words);
  HIP_TRY(a, copy_out(a, h.data(), sw.bitmap, words * sizeof(uint32_t)));
  uint64_t n = 0;
  for (uint64_t w = 0; w < n_win; ++w)
    if (h[w >> 5] >> (w & 31) & 1u) {
      if (n < cap) windows[n] = w;
      ++n;
    }
  *count = n;
  if (n > cap) return fail(a, who, std::to_string(n) + " windows are occupied, the caller's array holds " + std::to_string(cap));
  return DYN_OK;
}

int dyn_aligner_site_summary_fetch(dyn_aligner* a, uint64_t lo, uint64_t hi, uint64_t* n_rows, uint64_t* n_samples,
                                   uint64_t* dwell_sq, uint64_t* m1_lo, uint64_t* m1_hi, uint64_t* m2_lo, uint64_t* m2_hi,
                                   uint64_t totals[5]) {
  if (!a || !totals) return DYN_ERR_INVALID_ARGUMENT;
  uint64_t* cols[7] = {n_rows, n_samples, dwell_sq, m1_lo, m1_hi, m2_lo, m2_hi};
  if (lo < hi)
    for (uint64_t* c : cols)
      if (!c) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_range_quiet(a, "dyn_aligner_site_summary_fetch", lo, hi)) return rc;
  const uint64_t F = (uint64_t)dynk::SS_FIELDS;
  const Windows win(lo, hi - lo);
  std::vector<uint64_t> h(F * win.most + 1);
  for (auto [s0, cnt, o] : win) {
    const uint64_t* src = nullptr;  // (sparse: the window's ids looked up, their cells gathered -- an absent id: zeros)
    if (int rc = table_window(a, s0, cnt, win.most, 0, 1, &src)) return rc;
    HIP_TRY(a, copy_out(a, h.data(), src, F * cnt * sizeof(uint64_t)));
    for (uint64_t c = 0; c < cnt; ++c)
      for (uint64_t f = 0; f < F; ++f) cols[f][o + c] = h[F * c + f];
  }
  HIP_TRY(a, copy_out(a, totals, a->site.totals(), (uint64_t)dynk::SS_TOTALS * sizeof(uint64_t)));
  return DYN_OK;
}

int dyn_aligner_site_summary_reset(dyn_aligner* a) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_summary_quiet(a, "dyn_aligner_site_summary_reset")) return rc;
  SiteTable& t = a->site;
  HIP_TRY(a, hipMemsetAsync(t.table.p, 0, t.words() * sizeof(uint64_t), a->s_get));  // (the map's statistics with it)
  if (t.sparse()) HIP_TRY(a, hipMemsetAsync(t.keys.p, 0xFF, t.capacity * sizeof(uint32_t), a->s_get));  // no key left
  if (t.has_hist()) HIP_TRY(a, hipMemsetAsync(t.hist.p, 0, t.rows() * t.hist_width() * sizeof(uint32_t), a->s_get));
  HIP_TRY(a, hipStreamSynchronize(a->s_get));
  return DYN_OK;
}

// ---- the per-site histograms beside the table (site_summary_kernels.hpp) -------------------------------------------------------
int dyn_aligner_set_site_histogram(dyn_aligner* a, int bins, double lo, double hi) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_set_site_histogram";
  if (bins == 0) {  // off: the counters stay for the fetch
    std::lock_guard<std::mutex> lk(a->mu);
    a->opt.site_histogram = false;
    return DYN_OK;
  }
  // refused before the device is looked at: the same text on a handle without one
  if (bins < 2 || bins > dynk::SH_BINS_MAX) return fail(a, who, "bins " + std::to_string(bins) + " is not 0 (off) or 2 .. 254");
  if (!std::isfinite(lo) || !std::isfinite(hi) || !(lo < hi)) return fail(a, who, "lo and hi must be finite with lo < hi");
  const double inv_w = (double)bins / (hi - lo);  // one IEEE subtraction, one IEEE division
  if (!std::isfinite(inv_w) || !(inv_w > 0.0)) return fail(a, who, "hi - lo must be a finite width with a finite bins / (hi - lo)");
  std::unique_lock<std::mutex> lk(a->mu);
  SiteTable& t = a->site;
  if (!t.table.p) return fail(a, who, NO_TABLE);
  if (int rc = need_device(a)) return rc;
  if (t.hist.p && t.bins == (uint32_t)bins && t.lo == lo && t.hi == hi) {
    a->opt.site_histogram = true;
    return DYN_OK;
  }
  // other parameters
  if (int rc = retire_and_wait(a, lk, &JobOptions::site_histogram)) return rc;
  t.release_hist();
  if (!t.table.p || !t.num_sites) return fail(a, who, NO_TABLE);
  const uint64_t bytes = t.rows() * SiteTable::hist_width((uint32_t)bins) * sizeof(uint32_t);  // (a sparse table: capacity rows)
  const std::string what = "the histograms of " + std::to_string(t.rows()) + (t.sparse() ? " rows (" : " sites (") + std::to_string(bytes) + " bytes)";
  if (int rc = alloc_zeroed(a, who, what, "do not fit", {{&t.hist, bytes, 0}})) return rc;
  t.bins = (uint32_t)bins;
  t.lo = lo;
  t.hi = hi;
  t.inv_w = inv_w;
  a->opt.site_histogram = true;
  return DYN_OK;
}

int dyn_aligner_site_histogram_fetch(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint32_t* level, uint32_t* dwell) {
  if (!a || (site_lo < site_hi && (!level || !dwell))) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_histogram_quiet(a, "dyn_aligner_site_histogram_fetch", site_lo, site_hi)) return rc;
  const uint64_t B = (uint64_t)a->site.bins + 2, D = (uint64_t)dynk::SH_DWELL_BINS, H = B + D;
  const Windows win(site_lo, site_hi - site_lo);
  std::vector<uint32_t> h(H * win.most + 1);
  for (auto [s0, cnt, o] : win) {
    const unsigned int* src = nullptr;
    if (int rc = hist_window(a, s0, cnt, win.most, 0, 1, &src)) return rc;
    HIP_TRY(a, copy_out(a, h.data(), src, H * cnt * sizeof(uint32_t)));
    for (uint64_t c = 0; c < cnt; ++c) {
      std::memcpy(level + B * (o + c), h.data() + H * c, B * sizeof(uint32_t));
      std::memcpy(dwell + D * (o + c), h.data() + H * c + B, D * sizeof(uint32_t));
    }
  }
  return DYN_OK;
}

int dyn_aligner_site_quantiles(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, const double* probs, int n_probs, uint32_t* n,
                               uint32_t* rank, uint32_t* bin, uint32_t* below, uint32_t* in_bin) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_quantiles";
  if (!probs || n_probs < 1 || n_probs > dynk::SQ_PROBS_MAX) return fail(a, who, "n_probs " + std::to_string(n_probs) + " is not 1 .. 8");
  for (int q = 0; q < n_probs; ++q)
    if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) return fail(a, who, "probs[" + std::to_string(q) + "] is not in [0, 1]");
  if (site_lo < site_hi && (!n || !rank || !bin || !below || !in_bin)) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_histogram_quiet(a, who, site_lo, site_hi)) return rc;
  if (site_lo == site_hi) return DYN_OK;
  const uint64_t P = (uint64_t)n_probs;
  const Windows win(site_lo, site_hi - site_lo);
  HIP_TRY(a, a->site.quant.ensure((1 + 4 * P) * win.most * sizeof(uint32_t)));
  std::vector<uint32_t> h((1 + 4 * P) * win.most);
  dynk::SiteQuantiles sq{};
  sq.bins = a->site.bins;
  sq.n_probs = n_probs;
  for (int q = 0; q < n_probs; ++q) sq.probs[q] = probs[q];
  sq.out = a->site.quant.as<uint32_t>();
  for (auto [s0, cnt, o] : win) {
    if (int rc = hist_window(a, s0, cnt, win.most, 0, 1, &sq.hist)) return rc;
    sq.count = (uint32_t)cnt;
    dynk::launch_site_quantiles(sq, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, copy_out(a, h.data(), sq.out, (1 + 4 * P) * cnt * sizeof(uint32_t)));  // (behind the kernel on the same stream)
    std::memcpy(n + o, h.data(), cnt * sizeof(uint32_t));
    uint32_t* cols[4] = {rank, bin, below, in_bin};
    for (int f = 0; f < 4; ++f) std::memcpy(cols[f] + o * P, h.data() + cnt + (uint64_t)f * cnt * P, cnt * P * sizeof(uint32_t));
  }
  return DYN_OK;
}

// ---- two samples in one table: the exact add of host columns and the comparison of two windows (site_compare_kernels.hpp) ----
int dyn_aligner_site_summary_add(dyn_aligner* a, uint64_t lo, uint64_t hi, const uint64_t* n_rows, const uint64_t* n_samples,
                                 const uint64_t* dwell_sq, const uint64_t* m1_lo, const uint64_t* m1_hi, const uint64_t* m2_lo,
                                 const uint64_t* m2_hi, const uint64_t totals[5], const uint32_t* level, const uint32_t* dwell) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_summary_add";
  // refused before the device is looked at: the same text on a handle without one
  if ((level == nullptr) != (dwell == nullptr)) return fail(a, who, "level and dwell counters are given together or not at all");
  const uint64_t* cols[7] = {n_rows, n_samples, dwell_sq, m1_lo, m1_hi, m2_lo, m2_hi};
  if (lo < hi)
    for (const uint64_t* c : cols)
      if (!c) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = level ? site_histogram_quiet(a, who, lo, hi) : site_range_quiet(a, who, lo, hi)) return rc;
  if (lo == hi) return DYN_OK;  // an empty window touches nothing, the totals included
  SiteTable& t = a->site;
  const uint64_t F = (uint64_t)dynk::SS_FIELDS;
  const uint64_t B = (uint64_t)t.bins + 2, D = (uint64_t)dynk::SH_DWELL_BINS, H = level ? B + D : 0;
  const Windows win(lo, hi - lo);
  HIP_TRY(a, t.add.ensure(win.most * (F * sizeof(uint64_t) + H * sizeof(uint32_t))));
  std::vector<uint64_t> hc(F * win.most);
  std::vector<uint32_t> hh(H * win.most);
  dynk::SiteAdd sa{};
  sa.totals = t.totals();
  sa.cols = t.add.as<unsigned long long>();
  sa.width = (uint32_t)H;
  // a sparse table counts the sites that find no bucket in its map: this call's are those counted while it ran
  const unsigned long long* dropped_at = sa.totals + dynk::SS_TOTALS + dynk::SM_SITES_DROPPED;
  uint64_t dropped_before = 0, dropped = 0;
  if (t.sparse()) HIP_TRY(a, copy_out(a, &dropped_before, dropped_at, sizeof(uint64_t)));
  for (auto [s0, cnt, o] : win) {
    for (uint64_t c = 0; c < cnt; ++c)
      for (uint64_t f = 0; f < F; ++f) hc[F * c + f] = cols[f][o + c];
    HIP_TRY(a, hipMemcpyAsync(t.add.p, hc.data(), F * cnt * sizeof(uint64_t), hipMemcpyHostToDevice, a->s_get));
    sa.count = (uint32_t)cnt;
    if (level) {
      for (uint64_t c = 0; c < cnt; ++c) {
        std::memcpy(hh.data() + H * c, level + B * (o + c), B * sizeof(uint32_t));
        std::memcpy(hh.data() + H * c + B, dwell + D * (o + c), D * sizeof(uint32_t));
      }
      unsigned int* staged = reinterpret_cast<unsigned int*>(t.add.as<unsigned long long>() + F * cnt);
      HIP_TRY(a, hipMemcpyAsync(staged, hh.data(), H * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, a->s_get));
      sa.counters = staged;
    }
    sa.add_totals = (totals && s0 == lo) ? 1 : 0;  // the caller's totals once, with the first window
    for (int f = 0; f < dynk::SS_TOTALS; ++f) sa.totals_in[f] = sa.add_totals ? totals[f] : 0ull;
    if (t.sparse()) {  // the same staging, scattered into the rows of the window's ids (site_map_kernels.hpp)
      dynk::SiteScatter ssc{};
      ssc.keys = t.keys.as<uint32_t>();
      ssc.capacity = (uint32_t)t.capacity;
      ssc.stats = sa.totals + dynk::SS_TOTALS;
      ssc.acc = t.table.as<unsigned long long>();
      ssc.totals = sa.totals;
      ssc.hist = level ? t.hist.as<unsigned int>() : nullptr;
      ssc.cols = sa.cols;
      ssc.counters = sa.counters;
      ssc.width = sa.width;
      ssc.lo = (uint32_t)s0;
      ssc.count = sa.count;
      ssc.add_totals = sa.add_totals;
      for (int f = 0; f < dynk::SS_TOTALS; ++f) ssc.totals_in[f] = sa.totals_in[f];
      dynk::launch_site_scatter_add(ssc, a->s_get);
    } else {
      sa.acc = t.table.as<unsigned long long>() + F * s0;
      sa.hist = level ? t.hist.as<unsigned int>() + H * s0 : nullptr;
      dynk::launch_site_add(sa, a->s_get);
    }
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, hipStreamSynchronize(a->s_get));  // (the host vectors are filled again for the next window)
  }
  if (t.sparse()) HIP_TRY(a, copy_out(a, &dropped, dropped_at, sizeof(uint64_t)));
  if (dropped > dropped_before)
    return fail(a, who, std::to_string(dropped - dropped_before) + " sites found no bucket in the map of " + std::to_string(t.capacity) +
                            " rows and were dropped; the other sites were added", DYN_ERR_OUT_OF_MEMORY);
  return DYN_OK;
}

// ---- the table by content: the live rows as records, and records added by key (site_pack_kernels.hpp) -------------------------
int dyn_aligner_site_pack(dyn_aligner* a, uint64_t row_lo, uint64_t row_hi, uint64_t site_lo, uint64_t site_hi, uint64_t cap, uint32_t* site,
                          uint64_t* cells, uint32_t* level, uint32_t* dwell, uint64_t* count) {
  if (!a || !count) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_pack";
  // refused before the device is looked at: the same text on a handle without one
  if ((level == nullptr) != (dwell == nullptr)) return fail(a, who, "level and dwell counters are given together or not at all");
  if (cap && (!site || !cells)) return DYN_ERR_INVALID_ARGUMENT;
  *count = 0;
  if (row_lo > row_hi) return fail(a, who, "[" + std::to_string(row_lo) + ", " + std::to_string(row_hi) + ") is not a range of rows");
  if (site_lo > site_hi) return fail(a, who, "[" + std::to_string(site_lo) + ", " + std::to_string(site_hi) + ") is not a range of sites");
  if (row_lo == row_hi || site_lo == site_hi) return DYN_OK;  // an empty range touches nothing: no lock, no stream, no device
  // The table behind every ticket submitted before this call: the tickets in flight finish first (the setters' drain, with the
  // lock dropped while it waits -- a ticket may still be in front of its launch, where waiting for the streams would not see it),
  // then, under the lock again, both adding streams are waited for.
  std::unique_lock<std::mutex> lk(a->mu);
  if (Pipeline* pipe = a->pipe.get()) {
    lk.unlock();
    pipe->drain();
    lk.lock();
  }
  if (int rc = level ? site_histogram_quiet(a, who, 0, 0) : site_summary_quiet(a, who)) return rc;
  SiteTable& t = a->site;
  // (the two bounds below are the table's own: they can only be looked at where there is a table)
  if (!in_table(a, site_lo, site_hi)) return fail(a, who, no_range(a, site_lo, site_hi));
  if (row_hi > t.rows())
    return fail(a, who, "[" + std::to_string(row_lo) + ", " + std::to_string(row_hi) + ") is not a range of the table's " + std::to_string(t.rows()) + " rows");
  const uint64_t F = (uint64_t)dynk::SS_FIELDS;
  const uint64_t B = (uint64_t)t.bins + 2, D = (uint64_t)dynk::SH_DWELL_BINS, H = level ? B + D : 0;
  const Windows win(row_lo, row_hi - row_lo);
  // the scratch of the passes: the total, then a live mask and an offset per chunk of 64 rows
  const uint64_t chunks = (win.most + dynk::SPK_CHUNK_ROWS - 1) / dynk::SPK_CHUNK_ROWS;
  HIP_TRY(a, t.pack_scan.ensure(sizeof(uint64_t) * (1 + chunks) + sizeof(uint32_t) * chunks));
  dynk::SitePack sp{};
  sp.keys = t.sparse() ? t.keys.as<uint32_t>() : nullptr;
  sp.acc = t.table.as<unsigned long long>();
  sp.hist = level ? t.hist.as<unsigned int>() : nullptr;
  sp.width = (uint32_t)H;
  sp.site_lo = (uint32_t)site_lo;
  sp.site_hi = (uint32_t)site_hi;
  sp.total = t.pack_scan.as<unsigned long long>();
  sp.mask = sp.total + 1;
  sp.offset = reinterpret_cast<uint32_t*>(sp.mask + chunks);
  auto count_window = [&](uint64_t r0, uint64_t cnt, uint64_t* live) -> int {
    sp.row_lo = (uint32_t)r0;
    sp.count = (uint32_t)cnt;
    dynk::launch_site_pack(sp, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, copy_out(a, live, sp.total, sizeof(uint64_t)));  // (behind the two kernels on the same stream)
    return DYN_OK;
  };
  // the count of every window first: a caller whose arrays are too small gets the count and nothing else
  std::vector<uint64_t> live;
  uint64_t n = 0, most = 0;
  for (auto [r0, cnt, o] : win) {
    uint64_t c = 0;
    if (int rc = count_window(r0, cnt, &c)) return rc;
    live.push_back(c);
    n += c;
    most = std::max(most, c);
  }
  *count = n;
  if (n > cap) return fail(a, who, std::to_string(n) + " rows are live, the caller's arrays hold " + std::to_string(cap));
  if (n == 0) return DYN_OK;
  // the records of one window: cells, then counters, then ids (every section 4-byte aligned or better)
  // (headroom: a caller that walks the table window by window meets a new maximum often, and growing is hipFree + hipMalloc)
  HIP_TRY(a, t.pack.ensure(most * (F * sizeof(uint64_t) + H * sizeof(uint32_t) + sizeof(uint32_t)), 2.0));
  sp.cap = most;
  sp.out_cells = t.pack.as<unsigned long long>();
  sp.out_hist = reinterpret_cast<unsigned int*>(sp.out_cells + F * most);
  sp.out_site = sp.out_hist + H * most;
  std::vector<uint32_t> hh(H * most);
  uint64_t at = 0, w = 0;
  for (auto [r0, cnt, o] : win) {
    const uint64_t c = live[w++];
    if (c == 0) continue;
    if (live.size() > 1) {  // the scratch holds the last window's masks: this window's again
      uint64_t again = 0;
      if (int rc = count_window(r0, cnt, &again)) return rc;
      if (again != c) return fail(a, who, "the table changed while it was packed (a job was submitted from another thread)", DYN_ERR_DEVICE);
    }
    sp.row_lo = (uint32_t)r0;
    sp.count = (uint32_t)cnt;
    dynk::launch_site_pack_write(sp, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, hipMemcpyAsync(site + at, sp.out_site, c * sizeof(uint32_t), hipMemcpyDeviceToHost, a->s_get));
    if (level) HIP_TRY(a, hipMemcpyAsync(hh.data(), sp.out_hist, H * c * sizeof(uint32_t), hipMemcpyDeviceToHost, a->s_get));
    HIP_TRY(a, copy_out(a, cells + F * at, sp.out_cells, F * c * sizeof(uint64_t)));
    for (uint64_t i = 0; level && i < c; ++i) {
      std::memcpy(level + B * (at + i), hh.data() + H * i, B * sizeof(uint32_t));
      std::memcpy(dwell + D * (at + i), hh.data() + H * i + B, D * sizeof(uint32_t));
    }
    at += c;
  }
  return DYN_OK;
}

int dyn_aligner_site_summary_merge(dyn_aligner* a, uint64_t count, const uint32_t* site, uint64_t offset, const uint64_t* cells,
                                   const uint64_t totals[5], const uint32_t* level, const uint32_t* dwell) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_summary_merge";
  // refused before the device is looked at: the same text on a handle without one
  if ((level == nullptr) != (dwell == nullptr)) return fail(a, who, "level and dwell counters are given together or not at all");
  if (count && (!site || !cells)) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = level ? site_histogram_quiet(a, who, 0, 0) : site_summary_quiet(a, who)) return rc;
  if (count == 0 && !totals) return DYN_OK;  // nothing to add touches nothing
  SiteTable& t = a->site;
  for (uint64_t i = 0; i < count; ++i)  // refused before anything is added
    if (offset >= t.num_sites || site[i] >= t.num_sites - offset)
      return fail(a, who, "record " + std::to_string(i) + ": id " + std::to_string(site[i]) + " + offset " + std::to_string(offset) +
                              " is not below the table's " + std::to_string(t.num_sites) + " sites");
  const uint64_t F = (uint64_t)dynk::SS_FIELDS;
  const uint64_t B = (uint64_t)t.bins + 2, D = (uint64_t)dynk::SH_DWELL_BINS, H = level ? B + D : 0;
  const Windows win(0, count);  // (of records, not of ids)
  if (count) HIP_TRY(a, t.merge.ensure(win.most * (F * sizeof(uint64_t) + H * sizeof(uint32_t) + sizeof(uint32_t))));
  std::vector<uint32_t> hh(H * win.most);
  dynk::SiteMerge sm{};
  sm.keys = t.sparse() ? t.keys.as<uint32_t>() : nullptr;
  sm.capacity = (uint32_t)t.capacity;
  sm.totals = t.totals();
  sm.stats = t.sparse() ? sm.totals + dynk::SS_TOTALS : nullptr;
  sm.acc = t.table.as<unsigned long long>();
  sm.hist = level ? t.hist.as<unsigned int>() : nullptr;
  sm.width = (uint32_t)H;
  sm.offset = offset;
  sm.num_sites = t.num_sites;
  unsigned long long* d_cells = t.merge.as<unsigned long long>();
  unsigned int* d_counters = reinterpret_cast<unsigned int*>(d_cells + F * win.most);
  uint32_t* d_site = d_counters + H * win.most;
  sm.cells = d_cells;
  sm.counters = d_counters;
  sm.site = d_site;
  const unsigned long long* dropped_at = sm.totals + dynk::SS_TOTALS + dynk::SM_SITES_DROPPED;
  uint64_t dropped_before = 0, dropped = 0;
  if (t.sparse()) HIP_TRY(a, copy_out(a, &dropped_before, dropped_at, sizeof(uint64_t)));
  if (count == 0) {  // the totals alone (a rank that covered no site still counted its reads): one launch without records
    sm.add_totals = 1;
    for (int f = 0; f < dynk::SS_TOTALS; ++f) sm.totals_in[f] = totals[f];
    dynk::launch_site_merge(sm, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, hipStreamSynchronize(a->s_get));
    return DYN_OK;
  }
  for (auto [r0, cnt, o] : win) {
    HIP_TRY(a, hipMemcpyAsync(d_cells, cells + F * r0, F * cnt * sizeof(uint64_t), hipMemcpyHostToDevice, a->s_get));
    HIP_TRY(a, hipMemcpyAsync(d_site, site + r0, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, a->s_get));
    if (level) {
      for (uint64_t c = 0; c < cnt; ++c) {
        std::memcpy(hh.data() + H * c, level + B * (r0 + c), B * sizeof(uint32_t));
        std::memcpy(hh.data() + H * c + B, dwell + D * (r0 + c), D * sizeof(uint32_t));
      }
      HIP_TRY(a, hipMemcpyAsync(d_counters, hh.data(), H * cnt * sizeof(uint32_t), hipMemcpyHostToDevice, a->s_get));
    }
    sm.count = (uint32_t)cnt;
    sm.add_totals = (totals && r0 == 0) ? 1 : 0;  // the caller's totals once, with the first chunk
    for (int f = 0; f < dynk::SS_TOTALS; ++f) sm.totals_in[f] = sm.add_totals ? totals[f] : 0ull;
    dynk::launch_site_merge(sm, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, hipStreamSynchronize(a->s_get));  // (the host vector is filled again for the next chunk)
  }
  if (t.sparse()) HIP_TRY(a, copy_out(a, &dropped, dropped_at, sizeof(uint64_t)));
  if (dropped > dropped_before)
    return fail(a, who, std::to_string(dropped - dropped_before) + " sites found no bucket in the map of " + std::to_string(t.capacity) +
                            " rows and were dropped; the other sites were added", DYN_ERR_OUT_OF_MEMORY);
  return DYN_OK;
}

int dyn_aligner_site_compare(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint64_t other_lo, uint32_t* n_a, uint32_t* n_b,
                             uint64_t* level_num, uint32_t* level_at, int32_t* level_side, uint64_t* dwell_num, uint32_t* dwell_at,
                             int32_t* dwell_side) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_compare";
  if (site_lo < site_hi && (!n_a || !n_b || !level_num || !level_at || !level_side || !dwell_num || !dwell_at || !dwell_side))
    return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_histogram_quiet(a, who, site_lo, site_hi)) return rc;
  const uint64_t n = site_hi - site_lo;
  if (!other_in_table(a, other_lo, n)) return fail(a, who, no_other_window(a, other_lo, n));
  if (n == 0) return DYN_OK;
  const Windows win(site_lo, n);
  HIP_TRY(a, a->site.comp.ensure((uint64_t)dynk::SC_PAIR_BYTES * win.most));
  std::vector<uint64_t> h((uint64_t)dynk::SC_PAIR_BYTES / 8 * win.most);
  dynk::SiteCompare sc{};
  sc.bins = a->site.bins;
  sc.out = a->site.comp.as<unsigned long long>();
  for (auto [s0, cnt, o] : win) {  // (sparse: either window gathered into a slot of its own)
    if (int rc = hist_window(a, s0, cnt, win.most, 0, 2, &sc.hist_a)) return rc;
    if (int rc = hist_window(a, other_lo + o, cnt, win.most, 1, 2, &sc.hist_b)) return rc;
    sc.count = (uint32_t)cnt;
    dynk::launch_site_compare(sc, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, copy_out(a, h.data(), sc.out, (uint64_t)dynk::SC_PAIR_BYTES * cnt));  // (behind the kernel on the same stream)
    std::memcpy(level_num + o, h.data(), cnt * sizeof(uint64_t));
    std::memcpy(dwell_num + o, h.data() + cnt, cnt * sizeof(uint64_t));
    const uint32_t* w = reinterpret_cast<const uint32_t*>(h.data() + 2 * cnt);
    std::memcpy(n_a + o, w, cnt * sizeof(uint32_t));
    std::memcpy(n_b + o, w + cnt, cnt * sizeof(uint32_t));
    std::memcpy(level_at + o, w + 2 * cnt, cnt * sizeof(uint32_t));
    std::memcpy(dwell_at + o, w + 3 * cnt, cnt * sizeof(uint32_t));
    std::memcpy(level_side + o, w + 4 * cnt, cnt * sizeof(int32_t));
    std::memcpy(dwell_side + o, w + 5 * cnt, cnt * sizeof(int32_t));
  }
  return DYN_OK;
}

// ---- a two-component mixture per site pair, fitted on the device from the level counters (site_mixture_kernels.hpp) ----
int dyn_aligner_site_mixture(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint64_t other_lo, uint32_t max_iters, double tol,
                             uint32_t min_n, double* pi1, double* mu0, double* mu1, double* var0, double* var1, double* r_a, double* r_b,
                             uint32_t* n_a, uint32_t* n_b, uint32_t* out_a, uint32_t* out_b, uint32_t* iters, uint32_t* status) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_site_mixture";
  // refused before the device is looked at: the same text on a handle without one
  if (max_iters < 1 || max_iters > dynk::SM_MAX_ITERS) return fail(a, who, "max_iters " + std::to_string(max_iters) + " is not 1 .. 1024");
  if (!std::isfinite(tol) || !(tol >= 0.0)) return fail(a, who, "tol must be finite and >= 0");
  if (min_n < 2) return fail(a, who, "min_n " + std::to_string(min_n) + " is not >= 2");
  double* dcols[7] = {pi1, mu0, mu1, var0, var1, r_a, r_b};
  uint32_t* ucols[6] = {n_a, n_b, out_a, out_b, iters, status};
  if (site_lo < site_hi) {
    for (double* c : dcols)
      if (!c) return DYN_ERR_INVALID_ARGUMENT;
    for (uint32_t* c : ucols)
      if (!c) return DYN_ERR_INVALID_ARGUMENT;
  }
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_histogram_quiet(a, who, site_lo, site_hi)) return rc;
  const SiteTable& t = a->site;
  const uint64_t n = site_hi - site_lo;
  const bool one = other_lo == UINT64_MAX;
  if (!one && !other_in_table(a, other_lo, n)) return fail(a, who, no_other_window(a, other_lo, n));
  if (n == 0) return DYN_OK;
  const Windows win(site_lo, n);
  HIP_TRY(a, a->site.mix.ensure((uint64_t)dynk::SM_PAIR_BYTES * win.most));
  std::vector<double> h((uint64_t)dynk::SM_PAIR_BYTES / 8 * win.most);
  dynk::SiteMixture sm{};
  sm.exp_tab = reinterpret_cast<const uint64_t*>(a->d_sptab.as<dynmath::SoftplusNode>() + dynmath::SP_NODES + dynmath::EXP128_NODES);
  sm.bins = t.bins;
  sm.max_iters = max_iters;
  sm.min_n = min_n;
  sm.lo = t.lo;
  sm.w = (t.hi - t.lo) / (double)t.bins;  // one IEEE subtraction, one IEEE division
  sm.vfloor = (sm.w * sm.w) / 12.0;
  sm.tol_mu = tol * sm.w;
  sm.tol_pi = tol;
  sm.out = t.mix.as<double>();
  const int slots = one ? 1 : 2;
  for (auto [s0, cnt, o] : win) {
    if (int rc = hist_window(a, s0, cnt, win.most, 0, slots, &sm.hist_a)) return rc;
    if (!one)
      if (int rc = hist_window(a, other_lo + o, cnt, win.most, 1, slots, &sm.hist_b)) return rc;
    sm.count = (uint32_t)cnt;
    dynk::launch_site_mixture(sm, a->s_get);
    HIP_TRY(a, hipGetLastError());
    HIP_TRY(a, copy_out(a, h.data(), sm.out, (uint64_t)dynk::SM_PAIR_BYTES * cnt));  // (behind the kernel on the same stream)
    for (int f = 0; f < 7; ++f) std::memcpy(dcols[f] + o, h.data() + (uint64_t)f * cnt, cnt * sizeof(double));
    const uint32_t* w = reinterpret_cast<const uint32_t*>(h.data() + 7 * cnt);
    for (int f = 0; f < 6; ++f) std::memcpy(ucols[f] + o, w + (uint64_t)f * cnt, cnt * sizeof(uint32_t));
  }
  return DYN_OK;
}

// ---- the per-site model beside the table and its window calls (site_call_kernels.hpp) ---------------------------------------------
int dyn_aligner_set_site_model(dyn_aligner* a, uint64_t site_lo, uint64_t count, const double* pi1, const double* mu0, const double* mu1,
                               const double* var0, const double* var1, uint64_t* dropped) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  const char* who = "dyn_aligner_set_site_model";
  const double* cols[5] = {pi1, mu0, mu1, var0, var1};
  if (count)
    for (const double* c : cols)
      if (!c) return DYN_ERR_INVALID_ARGUMENT;
  if (dropped) *dropped = 0;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_summary_quiet(a, who)) return rc;
  SiteTable& t = a->site;
  if (!a->opt.site_summary) return fail(a, who, "dyn_aligner_set_site_summary(a, num_sites > 0) is off on this handle");
  if (site_lo > t.num_sites || count > t.num_sites - site_lo) return fail(a, who, no_range(a, site_lo, site_lo + count));
  if (count == 0) return DYN_OK;
  const uint64_t F = (uint64_t)dynk::SC_MODEL_FIELDS;
  if (!t.model.p) {  // the first upload: one row per table row, zeroed -- no row is set
    const uint64_t bytes = t.rows() * F * sizeof(double);
    const std::string what = "the site model of " + std::to_string(t.rows()) + (t.sparse() ? " rows (" : " sites (") + std::to_string(bytes) + " bytes)";
    if (int rc = alloc_zeroed(a, who, what, "does not fit", {{&t.model, bytes, 0}})) return rc;
  }
  const Windows win(site_lo, count);
  HIP_TRY(a, t.model_stage.ensure(win.most * F * sizeof(double) + sizeof(uint64_t)));
  unsigned long long* d_dropped = reinterpret_cast<unsigned long long*>(t.model_stage.as<double>() + win.most * F);
  HIP_TRY(a, hipMemsetAsync(d_dropped, 0, sizeof(uint64_t), a->s_get));
  std::vector<double> h(F * win.most);
  for (auto [s0, cnt, o] : win) {
    for (uint64_t c = 0; c < cnt; ++c)
      for (uint64_t f = 0; f < F; ++f) h[F * c + f] = cols[f][o + c];
    if (t.sparse()) {  // staged, then scattered into the rows of the window's ids
      HIP_TRY(a, hipMemcpyAsync(t.model_stage.p, h.data(), F * cnt * sizeof(double), hipMemcpyHostToDevice, a->s_get));
      dynk::SiteModelScatter ms{t.keys.as<uint32_t>(), (uint32_t)t.capacity, t.totals() + dynk::SS_TOTALS, t.model.as<double>(),
                                t.model_stage.as<double>(), (uint32_t)s0, (uint32_t)cnt, d_dropped};
      dynk::launch_site_model_scatter(ms, a->s_get);
      HIP_TRY(a, hipGetLastError());
    } else {
      HIP_TRY(a, hipMemcpyAsync(t.model.as<double>() + F * s0, h.data(), F * cnt * sizeof(double), hipMemcpyHostToDevice, a->s_get));
    }
    HIP_TRY(a, hipStreamSynchronize(a->s_get));  // (the host vector is filled again for the next window)
  }
  if (t.sparse() && dropped) HIP_TRY(a, copy_out(a, dropped, d_dropped, sizeof(uint64_t)));
  return DYN_OK;
}

int dyn_aligner_site_model_reset(dyn_aligner* a) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_summary_quiet(a, "dyn_aligner_site_model_reset")) return rc;
  SiteTable& t = a->site;
  if (!t.model.p) return DYN_OK;
  HIP_TRY(a, hipMemsetAsync(t.model.p, 0, t.rows() * dynk::SC_MODEL_FIELDS * sizeof(double), a->s_get));  // (a sparse map keeps its keys)
  HIP_TRY(a, hipStreamSynchronize(a->s_get));
  return DYN_OK;
}

int dyn_aligner_site_model_fetch(dyn_aligner* a, uint64_t lo, uint64_t hi, double* pi1, double* mu0, double* mu1, double* var0, double* var1) {
  if (!a) return DYN_ERR_INVALID_ARGUMENT;
  double* cols[5] = {pi1, mu0, mu1, var0, var1};
  if (lo < hi)
    for (double* c : cols)
      if (!c) return DYN_ERR_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lk(a->mu);
  if (int rc = site_range_quiet(a, "dyn_aligner_site_model_fetch", lo, hi)) return rc;
  SiteTable& t = a->site;
  const uint64_t F = (uint64_t)dynk::SC_MODEL_FIELDS;
  if (!t.model.p) {  // never uploaded: no row is set
    for (double* c : cols)
      if (lo < hi) std::fill(c, c + (hi - lo), 0.0);
    return DYN_OK;
  }
  const Windows win(lo, hi - lo);
  std::vector<double> h(F * win.most + 1);
  if (t.sparse() && hi > lo) HIP_TRY(a, t.model_stage.ensure(win.most * F * sizeof(double) + sizeof(uint64_t)));
  for (auto [s0, cnt, o] : win) {
    const double* src = t.model.as<double>() + F * s0;
    if (t.sparse()) {  // the window's ids looked up, their rows gathered -- an absent id: zeros
      dynk::SiteModelGather mg{t.keys.as<uint32_t>(), (uint32_t)t.capacity, t.model.as<double>(), (uint32_t)s0, (uint32_t)cnt, t.model_stage.as<double>()};
      dynk::launch_site_model_gather(mg, a->s_get);
      HIP_TRY(a, hipGetLastError());
      src = t.model_stage.as<double>();
    }
    HIP_TRY(a, copy_out(a, h.data(), src, F * cnt * sizeof(double)));  // (behind the kernel on the same stream)
    for (uint64_t c = 0; c < cnt; ++c)
      for (uint64_t f = 0; f < F; ++f) cols[f][o + c] = h[F * c + f];
  }
  return DYN_OK;
}

}  // extern "C"

namespace dyneng {

int take_staged_sites(dyn_aligner* a, const char* api, uint64_t n_reads, const uint64_t* seq_offsets, const uint32_t** ids) {
  *ids = nullptr;
  SiteTable& t = a->site;
  if (!t.staged) return DYN_OK;
  const uint32_t* p = t.staged_ids;
  const uint64_t count = t.staged_count;
  t.staged = false;
  t.staged_ids = nullptr;
  t.staged_count = 0;
  const uint64_t span = (n_reads && seq_offsets) ? seq_offsets[n_reads] - seq_offsets[0] : 0;
  if (count != span)
    return fail(a, api, "dyn_aligner_stage_site_ids staged " + std::to_string(count) + " ids, the batch's sequences hold " + std::to_string(span) + " characters");
  *ids = p;
  return DYN_OK;
}

}  // namespace dyneng
