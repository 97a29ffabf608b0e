// engine.hpp -- host-side state shared by the C-ABI entry points (dynamont_mi.cpp) and the
// asynchronous batch pipeline (async_engine.cpp).
//
// The reference keeps its worker processes permanently fed (src/dynamont/segmentation/segment.py:
// 301-325: a multiprocessing pool over generate_jobs with a listener process draining results).
// The GPU counterpart of that is a three-stage pipeline per handle:
//   front thread : validateInput + sequenceToKmers of batch k+1, staging into pinned memory, H2D on
//                  the copy-in stream, kernel launches on the compute stream (no host sync)
//   GPU          : kernels of batch k (compute stream), D2H of batch k-1 (copy-out stream)
//   back thread  : unpack of batch k-1 into the caller's columns
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/dynamont_mi.h"
#include "nt_kernels.hpp"
#include "pore_model.hpp"

namespace dyneng {

// Recycles device and pinned-host allocations of finished batches: hipFree synchronises the whole
// device and hipHostMalloc of a 160 MB buffer costs tens of milliseconds, either of which would
// stall a pipeline that has other batches in flight. Sizes are rounded up to a granule so that a
// stream of batches of slightly different size keeps hitting the same buffers.
struct BufCache {
  std::mutex m;
  std::multimap<size_t, void*> dev, pin;
  static size_t round_up(size_t want);
  hipError_t take(bool pinned, size_t want, void** p, size_t* got);
  void give(bool pinned, void* p, size_t bytes);
  void purge();  // frees everything (device idle)
  // Handle destruction: what the cache holds is PARKED for the next handle on that device instead of freed (hipFree /
  // hipHostFree of a dozen batches' buffers: 0.2 s at the end of a run; allocating them again: as much at the start of the
  // next). Bounded; dyn_release_cached_memory() frees what is parked, DYN_NO_POOL_CACHE=1 switches parking off.
  void park(int device);
  int device = -1;  // set by the handle: take() looks at the device's parked buffers before it allocates
  // set by the handle: true while a resident session is open. purge() frees with hipFree, which waits for the whole device --
  // i.e. for resident waves that only leave when the handle (whose lock the caller of take() holds) closes their session. An
  // allocation that fails meanwhile is reported; alloc_batch_buffers quiesces the session, purges and tries again.
  const std::atomic<bool>* session_open = nullptr;
};

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  BufCache* cache = nullptr;  // nullptr: grow-only buffer owned by the handle (lattice pools)
  // grow-only. `headroom` > 1 over-allocates when the buffer has to grow: releasing and re-allocating
  // a 70 GB lattice pool costs 4-5 s on an MI355X (measured, tools/batch_latency.py), which a stream
  // of batches of slightly different size would otherwise pay every time a new maximum shows up.
  hipError_t ensure(size_t want, double headroom = 1.0);
  void release();
  template <class T> T* as() const { return static_cast<T*>(p); }
};

struct PinnedBuf {
  void* p = nullptr;
  size_t bytes = 0;
  BufCache* cache = nullptr;
  hipError_t ensure(size_t want);
  void release();
  template <class T> T* as() const { return static_cast<T*>(p); }
};

// Small persistent worker pool for the host stages that are plain memory work (staging copies into
// pinned memory, rows -> columns unpack, k-mer coding).
class HelperPool {
 public:
  explicit HelperPool(int n_threads);
  ~HelperPool();
  // fn(task) for task in [0, n_tasks); returns when all are done. The calling thread takes part.
  void parallel_for(int n_tasks, const std::function<void(int)>& fn);
  int size() const { return (int)workers_.size() + 1; }

 private:
  void worker();
  std::vector<std::thread> workers_;
  std::mutex m_, call_m_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<void(int)>* fn_ = nullptr;
  int next_ = 0, n_ = 0, active_ = 0;
  uint64_t gen_ = 0;
  bool stop_ = false;
};

struct Pipeline;

// ---- the resident read queue of a handle (nt_kernels.hpp: k_session) -------------------------------------------------
// A SESSION is one launch of resident waves on the handle's session stream (a CU-masked stream: it owns its hardware
// queue, so the small kernels and copies that feed the waves can never queue up behind them -- tools/ubench/resident_probe).
// The pipeline's front thread opens one when an align(calc=true) ticket arrives whose reads fit a static arena per wave,
// publishes that ticket and every later one that fits, and the session is closed when the pipeline has run dry (or a
// ticket of another kind must use the lattice pool). Two control blocks alternate, so that a new session can be set up
// while the last waves of the previous one are leaving.
constexpr uint32_t SESSION_RING = 1024;        // tickets per session (the ring is never reused within one)
constexpr uint64_t SESSION_MIN_READS = 512;    // a session is OPENED only for a ticket of at least this many reads
constexpr uint32_t SESSION_FLAGS = 4096;       // completion words in pinned host memory (a ring: far more than tickets in flight)
struct Session {
  bool open = false;
  bool mixed = false;           // the kernel variant that carries the certified sweeps
  int blk = 0;                  // control block / ticket ring in use
  uint32_t published = 0;       // tickets of the open session
  uint32_t next_base = 0;       // global read index of the next ticket's first read
  int log_r = 8;
  uint32_t arena_pages = 0;     // lattice pages per wave (layout 0); paged layouts: the most a read may need
  int layout = 0;               // 0: an arena per wave; 1: pages shared through the free list; 2: shared pages, posteriors in place
  uint32_t n_pages = 0;         // pages of the pool
  uint32_t n_waves = 0;
  uint64_t cells = 0, reads = 0, tickets = 0;   // of the open session
  bool pending[2] = {false, false};             // a session ran on this block and its statistics have not been collected
  uint64_t pend_cells[2] = {0, 0}, pend_reads[2] = {0, 0}, pend_tickets[2] = {0, 0};
  uint32_t pend_waves[2] = {0, 0};
  hipEvent_t ev_begin[2] = {nullptr, nullptr}, ev_end[2] = {nullptr, nullptr};
  uint64_t flag_seq = 0;        // next completion word
  // which session runs (or ran last) on a control block: a ticket remembers its session's number, and a block that has moved on
  // to a later session while the ticket is incomplete has LOST it (wait_resident -> session_recover)
  std::atomic<uint64_t> blk_gen[2] = {{0}, {0}};
  uint64_t gen = 0;
};

// ---- the opt-in switches of a handle, as a job reads them ------------------------------------------------------------------
// dyn_aligner::opt is what the dyn_aligner_set_<switch> calls last said; dyn_batch::want is what ONE job took of it at its
// submission (resolve_job_options: masked by the job's kind and the handle's mode, refused where two switches do not combine).
struct JobOptions {
  bool event_stats = false;     // dyn_aligner_set_event_stats
  int rescale_iters = 0;        // dyn_aligner_set_rescale (0 .. 8)
  bool kmer_summary = false;    // dyn_aligner_set_kmer_summary
  bool site_summary = false;    // dyn_aligner_set_site_summary (num_sites > 0)
  bool site_histogram = false;  // dyn_aligner_set_site_histogram (bins > 0); counts only where site_summary does
  bool band_margin = false;     // dyn_aligner_set_band_margin
  int segment_scores = 0;       // dyn_aligner_set_segment_scores (window, 0 = off)
  int border_confidence = 0;    // dyn_aligner_set_border_confidence (window, 0 = off)
  double border_interval = 0;   // dyn_aligner_set_border_interval (mass, 0 = off)
  bool soft_levels = false;     // dyn_aligner_set_soft_levels
  bool site_calls = false;      // dyn_aligner_set_site_calls; needs site_summary
  int posterior_samples = 0;    // dyn_aligner_set_posterior_samples (count, 0 = off)
  uint64_t sample_seed = 0;     // ... and its seed
  uint32_t auto_guide_hw = 0, auto_guide_rounds = 8;               // dyn_aligner_set_auto_guide (half width, 0 = off; alignments per read)
  uint32_t rescue_margin = 0, rescue_hw = 0, rescue_rounds = 8;    // dyn_aligner_set_guide_rescue (minimum margin; half width, 0 = off; alignments)
  // May tickets x and y share ONE launch (Pipeline::merge)? Three kinds of fields:
  //   launch-wide: event_stats, rescale_iters, segment_scores, border_confidence, border_interval, soft_levels, site_calls -- one value per
  //                launch, so the members must agree; the launch's batch takes them from its first member
  //   per-ticket:  kmer_summary, site_summary, site_histogram, band_margin -- not compared: the launch's batch lists the read ranges of the members that asked
  //   alone:       posterior_samples (the read's index in its OWN ticket keys the random stream), auto_guide_hw (a guide of its own
  //                and the banded-lattice kernel), rescue_hw (its list of reads to re-align is its own) -- such a ticket never merges
  bool merges() const { return posterior_samples == 0 && auto_guide_hw == 0 && rescue_hw == 0; }
  bool same_launch(const JobOptions& y) const {
    return event_stats == y.event_stats && rescale_iters == y.rescale_iters && segment_scores == y.segment_scores &&
           border_confidence == y.border_confidence && border_interval == y.border_interval && soft_levels == y.soft_levels && site_calls == y.site_calls;
  }
  // the launch-wide part alone: what the batch of a merged launch runs under
  JobOptions launch_wide() const {
    JobOptions g;
    g.event_stats = event_stats;
    g.rescale_iters = rescale_iters;
    g.segment_scores = segment_scores;
    g.border_confidence = border_confidence;
    g.border_interval = border_interval;
    g.soft_levels = soft_levels;
    g.site_calls = site_calls;
    return g;
  }
};

// the per-site histograms as a job sees them (dyn_aligner_set_site_histogram): taken at its submission, beside the table's address
struct SiteHist {
  unsigned int* p = nullptr;  // [num_sites][bins + 2 + 16] uint32; nullptr: off
  uint32_t bins = 0;
  double lo = 0.0, inv_w = 0.0;
};
// the map of a sparse table as a job sees it (dyn_aligner_set_site_summary_sparse): taken at its submission likewise
struct SiteMap {
  uint32_t* keys = nullptr;  // [capacity]; nullptr: the table is dense
  uint64_t capacity = 0;
};

// ---- the per-site table of a handle and everything kept beside it (dyn_aligner::site; the calls: site_table.cpp) ---------------
struct SiteTable {
  // the table (site_summary_kernels.hpp): [7 rows() + 5] u64, allocated and zeroed by dyn_aligner_set_site_summary(a, num_sites > 0),
  // kept until the setter names another size; a job snapshots pointer and size at its submission
  DevBuf table;
  uint64_t num_sites = 0;
  // the sparse mode (dyn_aligner_set_site_summary_sparse, site_map.hpp): capacity > 0, keys the [capacity] uint32 keys of the map,
  // table [7 capacity + 5 + 3] u64 (the map's three statistics behind the totals), the histograms capacity rows; num_sites stays
  // the bound of the ids. gather: the dense scratch the window calls gather into (one or two windows of what the call reads)
  DevBuf keys;
  uint64_t capacity = 0;
  DevBuf gather;
  // the per-site model beside the table (dyn_aligner_set_site_model, site_call_kernels.hpp): [rows()][5] f64 pi1, mu0, mu1, var0, var1,
  // allocated and zeroed by the first upload, released with the table; a job snapshots the pointer at its submission. model_stage:
  // one window's staged rows per call (and, behind them, the counter of a sparse upload's dropped rows)
  DevBuf model, model_stage;
  // the per-site histograms beside the table: [rows()][bins + 2 + 16] u32, allocated and zeroed by dyn_aligner_set_site_histogram(a,
  // bins > 0, lo, hi), kept (bins = 0 only stops the counting) until that setter names other parameters or the table another size
  DevBuf hist;
  uint32_t bins = 0;
  double lo = 0.0, hi = 0.0, inv_w = 0.0;
  // one window's staging per call, each a buffer of its own: growing a buffer of the handle's is hipFree + hipMalloc, and hipFree
  // waits for the whole device -- calls of different sizes must not free one another's staging under an open resident session
  DevBuf quant;  // dyn_aligner_site_quantiles: one window's output
  DevBuf comp;   // dyn_aligner_site_compare: one window's output
  DevBuf mix;    // dyn_aligner_site_mixture: one window's output
  DevBuf add;    // dyn_aligner_site_summary_add: one window's columns and counters
  DevBuf pack;   // dyn_aligner_site_pack: one window's records (sized from the window's live count)
  DevBuf pack_scan;  // ... and its live masks, offsets and total, which have to outlive the growing of `pack` between the passes
  DevBuf merge;  // dyn_aligner_site_summary_merge: one chunk's staged records
  // dyn_aligner_stage_site_ids: the caller's ids for the NEXT batch-creating call on this handle (consumed by it, whatever its outcome)
  const uint32_t* staged_ids = nullptr;
  uint64_t staged_count = 0;
  bool staged = false;

  bool sparse() const { return capacity != 0; }
  // rows of the table and of its histograms: the capacity of a sparse table, the id space of a dense one
  uint64_t rows() const { return capacity ? capacity : num_sites; }
  // the table's words: the cells, the totals and, behind a sparse table, the map's statistics
  static uint64_t words(uint64_t rows, bool sparse) {
    return (uint64_t)dynk::SS_FIELDS * rows + (uint64_t)dynk::SS_TOTALS + (sparse ? (uint64_t)dynk::SM_STATS : 0);
  }
  uint64_t words() const { return words(rows(), sparse()); }
  unsigned long long* totals() const { return table.as<unsigned long long>() + (uint64_t)dynk::SS_FIELDS * rows(); }
  // uint32 counters per site: under, the level bins, over, the dwell bins
  static uint64_t hist_width(uint32_t bins) { return (uint64_t)bins + 2 + (uint64_t)dynk::SH_DWELL_BINS; }
  uint64_t hist_width() const { return hist_width(bins); }
  bool has_hist() const { return hist.p && bins; }
  // the histograms a job submitted now counts into (nothing while the switch is off)
  SiteHist hist_now(bool on) const {
    SiteHist h;
    if (on && has_hist()) {
      h.p = hist.as<unsigned int>();
      h.bins = bins;
      h.lo = lo;
      h.inv_w = inv_w;
    }
    return h;
  }
  SiteMap map_now() const {
    SiteMap m;
    if (capacity && keys.p) {
      m.keys = keys.as<uint32_t>();
      m.capacity = capacity;
    }
    return m;
  }
  // what dyn_aligner_set_mem_budget counts against the table: itself, its histograms, a sparse table's map and gather scratch
  uint64_t held_bytes() const { return table.bytes + hist.bytes + keys.bytes + gather.bytes + model.bytes; }
  // the occupancy bitmap of dyn_aligner_site_map_windows lives in the quantiles' staging: every window call runs under the
  // handle's lock on s_get, so no two of them use it at once
  DevBuf& window_bitmap() { return quant; }
  void release_hist() {
    hist.release();
    bins = 0;
  }
  // the table, its map and scratch and its histograms (the setter, before another size; the staging stays)
  void release_table() {
    table.release();
    keys.release();
    gather.release();
    model.release();
    num_sites = 0;
    capacity = 0;
    release_hist();
  }
  void release() {
    release_table();
    for (DevBuf* d : {&quant, &comp, &mix, &add, &model_stage, &pack, &pack_scan, &merge}) d->release();
  }
};

// ---- the per-segment outputs a job may add to its rows (one fetcher, one out-struct and one CSV flag each) ---------------------
enum Output { OUT_LEVELS, OUT_SCORES, OUT_BORDERS, OUT_INTERVALS, OUT_SOFT, OUT_SITE_CALLS, OUT_SAMPLES, OUT_COUNT };
struct OutputBuf {
  DevBuf d;       // OUT_LEVELS [3][capacity] f64 mean / stdev / median (event_stats.hip); OUT_SCORES [4][capacity] f64 median_delta /
                  // mad_delta / homogeneity / scratch (segment_scores.hip); OUT_BORDERS [2][capacity] f64 (border_kernels.hpp);
                  // OUT_INTERVALS [2][capacity] f64 mean / sd, then [2][capacity] u32 lo / hi (interval_kernels.hpp); OUT_SOFT [3][capacity] f64
                  // weight / sum / sumsq (soft_level_kernels.hpp); OUT_SITE_CALLS [2][capacity] f64 site_probability / site_z
                  // (site_call_kernels.hpp); OUT_SAMPLES
                  // [count][capacity] u32 sample starts, then [n] u32 dead samples (sample_kernels.hpp)
  int ready = 0;  // the last job computed the columns into d (OUT_SAMPLES: the count it sampled)
};
struct OutputDesc {
  uint32_t row_bytes;       // of d per segment row (OUT_SAMPLES: per sample; its [n] dead counts come on top)
  const char* fetch;        // the C-ABI fetcher, as its messages name it
  const char* out_struct;   // ... and its out-struct
  const char* setter_hint;  // the call that would have switched the output on
  uint32_t csv_flag;        // the dyn_csv_sink_open_ex flag that writes it
  const char* csv_what;     // ... as the sink's refusal names it
};
extern const OutputDesc OUTPUTS[OUT_COUNT];  // dynamont_mi.cpp

}  // namespace dyneng

struct dyn_aligner {
  dynhost::PoreModel model;
  int device = -1;
  bool host_only = false;
  int threads = 1;
  hipStream_t stream = nullptr;  // compute stream: every kernel of every batch of this handle, in submission order
  hipStream_t s_in = nullptr;    // H2D of the asynchronous pipeline
  hipStream_t s_out = nullptr;   // D2H of the asynchronous pipeline
  hipStream_t s_get = nullptr;   // the getters' copies (dyn_batch_fetch, _fetch_train, _signals): non-blocking, so that they do
                                 // not wait -- as a null-stream hipMemcpy would -- for a resident session that later tickets keep open
  dyneng::DevBuf d_model;
  dyneng::DevBuf d_sptab;  // softplus table (dp_math.hpp), staged into LDS by every DP workgroup
  uint64_t mem_budget = 0;
  int strict_mode = 1;  // dyn_aligner_set_strict: reads with a structural tie run bit for bit by default
  bool train_zcheck = false;  // dyn_aligner_set_train_zcheck
  // DYN_LPE_STORE_FLOOR, read once when the handle is created (debugging): `dense`, or the floor below which the forward
  // sweep does not store a lane group's float LPE (lpe_liveness.hpp)
  float lpe_floor = -750.0f;
  bool lpe_dense = false;
  dyneng::JobOptions opt;  // the dyn_aligner_set_<switch> calls write here; every batch / ticket takes its own copy at its submission
  // queue head + lattice arenas of the self-guided tickets (band_reads.hip): grow-only, the handle's, shared by every such ticket
  // in stream order (launch.cpp, enqueue_job) and released with the handle
  dyneng::DevBuf band_arena;
  dyneng::DevBuf d_ksum;      // [6 num_kmers + 4] u64: the per-k-mer accumulator and its totals (kmer_summary_kernels.hpp),
                              // allocated and zeroed by the first dyn_aligner_set_kmer_summary(a, 1)
  dyneng::SiteTable site;  // the per-site table, its map, histograms, staging and staged ids (site_table.cpp)
  bool ntk = false;     // created with mode "resquiggle" / "ntk"
  std::string last_error;
  // grow-only lattice workspace pool, reused across batches (only ever touched by work on `stream`,
  // whose order serialises the batches that share it)
  dyneng::DevBuf ws, lpe, bits;      // page pool of the read queue (nt_kernels.hpp, PagePool)
  dyneng::DevBuf free_list, ctl;     // its free-page stack and control words
  int n_cus = 256;                   // compute units: one persistent 4-wave workgroup each
  dyneng::PinnedBuf h_rows;  // staging of the synchronous dyn_batch_fetch
  dyneng::BufCache cache;
  // serialises GPU enqueue work on this handle between the caller's thread and the pipeline threads
  std::mutex mu;
  std::unique_ptr<dyneng::Pipeline> pipe;  // started by the first asynchronous submit
  // the resident read queue (guarded by mu)
  hipStream_t s_session = nullptr;   // CU-masked: a hardware queue of its own; nullptr = no sessions on this handle
  int sess_cus = 0;                  // CUs in its mask = workgroups of a session (n_cus minus what dyn_aligner_set_session_mode reserves)
  dyneng::DevBuf sess_ctl[2], sess_ring[2];
  dyneng::DevBuf sess_anchor;        // out_base of k_session: the address the ticket records' output offsets count from
  std::atomic<bool> sess_open_hint{false};  // mirrors sess.open for readers that do not hold mu
  std::atomic<bool> sess_enabled{false};    // mirrors s_session != nullptr likewise (the pipeline's front thread asks under ITS lock)
  std::mutex err_mu;                        // last_error is written by the caller's thread AND by the pipeline threads
  uint32_t* sess_flags = nullptr;    // [SESSION_FLAGS] pinned, coherent
  dyneng::PinnedBuf sess_hctl;       // D2H target of a control block
  dyneng::Session sess;
  dyn_session_stats sess_total{};    // closed and collected sessions
  uint64_t sess_idle_split[4] = {0, 0, 0, 0};  // wave-cycles: before a wave's first read, of which pages, last turn, longest last turn
  uint64_t sess_page_wait_cycles = 0;  // part of sess_total.wave_cycles_idle: waves of PAGED sessions getting their pages
  // the idle watchdog of the resident waves, seconds (DYN_SESSION_IDLE_S)
  double sess_idle_s = 20.0;
};

namespace dyneng {
// what dyn_aligner_set_mem_budget leaves once the per-site table and what it holds beside it are taken off (0: no budget was set)
inline uint64_t mem_budget_left(const dyn_aligner* a) {
  if (!a->mem_budget) return 0;
  const uint64_t taken = a->site.held_bytes();
  return a->mem_budget > taken ? a->mem_budget - taken : 1;
}
// what a session is launched with (session_choose, session.cpp)
struct SessionGeom {
  bool ok = false;
  int layout = 0, log_r = 8;
  uint32_t arena_pages = 0;   // layout 0: per wave; paged: the most one read may need
  uint32_t n_pages = 0;       // of the pool
};
}  // namespace dyneng

struct HostRead {
  uint64_t S = 0, L = 0, kc = 0;
  uint64_t sig_off = 0, flat_off = 0 /* into kmers / per-column tables */, seg_off = 0;
  int32_t status = 0;
  char bad = 0;
  bool wide = false;  // half band above the register sweeps' 223: the read takes the banded-lattice kernel (band_reads.hip)
};

enum class DynJob { AlignZ, AlignFull, Train };

// P1/P2 on the device (dyn_batch_create_raw / dyn_batch_*_raw_async): the batch's samples arrive as RAW slices
struct RawSource {
  const void* raw = nullptr;   // concatenated [start:end) slices; scattered: a table of n_reads pointers, one per slice
  bool scattered = false;
  // vbz: the samples arrive as POD5 signal chunks still compressed (VBZ); read i = chunks [vbz_read_off[i], vbz_read_off[i+1])
  // decoded back to back, of which the slice [vbz_skip[i], vbz_skip[i] + length_i) is the read's signal
  bool vbz = false;
  const void* const* vbz_chunks = nullptr;
  const uint64_t* vbz_bytes = nullptr;
  const uint32_t* vbz_samples = nullptr;
  const uint64_t* vbz_read_off = nullptr;
  const uint64_t* vbz_skip = nullptr;
  int dtype = 0;               // 0 float32, 1 int16, 2 float64, 3 int16 ADC + per-read float32 calibration
  const float* cal_offset = nullptr;  // dtype 3: picoampere = (adc + cal_offset) * cal_scale, in float32
  const float* cal_scale = nullptr;
  const double* shift = nullptr;
  const double* scale = nullptr;
  int window = 3;
  double n_sigmas = 3.0;
  int compute_f32 = 0;
  size_t elem_size() const { return dtype == 0 ? 4 : (dtype == 1 || dtype == 3) ? 2 : 8; }
};

namespace dyneng {
struct BatchGroup;
}

struct dyn_batch {
  dyn_aligner* a = nullptr;
  uint64_t n = 0;
  std::vector<HostRead> reads;
  dyneng::PinnedBuf h_kmers;   // flat int32 codes, ok reads only
  dyneng::PinnedBuf h_sites;   // flat uint32 site ids of the output rows, ok reads only (row j of a read: the id of base j + k / 2);
                               // filled by host_prepare when the batch has ids (has_sites)
  uint64_t capacity = 0;       // sum of kc over ALL reads with L >= k (segment rows)
  uint64_t total_cols = 0;     // sum of kc over ok reads
  uint32_t max_T = 0, max_N = 0;
  dyneng::DevBuf d_sig, d_kmers, d_par, d_state, d_rows, d_segrow, d_medhi, d_medlo, d_descs;
  dyneng::DevBuf d_colw, d_cols1, d_cols2, d_trans, d_pooled, d_poolwork, d_pooltemp;
  dyneng::DevBuf d_pp, d_pathn;                // per-row path arrays (traceback -> k_median / k_final)
  // what the handle's switches said when this batch / ticket was submitted (resolve_job_options)
  dyneng::JobOptions want;
  // the per-segment outputs (dyneng::Output), when asked for: the columns and whether the last job computed them
  dyneng::OutputBuf out[dyneng::OUT_COUNT];
  // per-read rescaling (rescale.hip, dyn_aligner_set_rescale)
  dyneng::DevBuf d_sig0;                       // the preprocessed signal x0, kept while d_sig holds a rescaled one
  dyneng::DevBuf d_rs;                         // [n] dynk::RescaleState | [capacity] row means of the fit (scratch)
  bool rs_ready = false;                       // the last job ran its passes: d_rs holds the per-read transforms
  bool sig0_kept = false;                      // d_sig0 holds x0 (a synchronous batch aligned again starts from it)
  uint64_t sig0_len = 0;                       // samples kept in d_sig0
  int n_passes = 1;                            // alignment passes of the last job (h_stats holds one record each)
  // per-k-mer summary and band-margin diagnostics (want.kmer_summary, want.band_margin): a merged launch's batch lists the read
  // ranges of the members that asked (JobOptions::same_launch does not look at the two switches)
  std::vector<std::pair<uint32_t, uint32_t>> ks_ranges, bm_ranges;
  // per-site summary (want.site_summary): the caller's per-base ids, packed like the sequences (nullptr: none staged -- the job
  // adds nothing), the per-row ids on the device, the handle's table as it stood at submission, and for a merged launch the read
  // ranges of the members that asked AND staged ids
  const uint32_t* in_site_ids = nullptr;
  bool has_sites = false;
  dyneng::DevBuf d_sites;
  unsigned long long* ss_table = nullptr;
  uint64_t ss_num_sites = 0;
  dyneng::SiteMap ss_map;  // the map of a sparse table as it stood at submission (keys == nullptr: dense)
  const double* ss_model = nullptr;  // the per-site model as it stood at submission (nullptr: none uploaded; want.site_calls reads it)
  // the site calls of a merged launch (want.site_calls is launch-wide): every member's read range with the model IT snapshot
  struct SiteCallRange {
    uint32_t lo, hi;
    const double* model;
  };
  std::vector<SiteCallRange> sc_ranges;
  std::vector<std::pair<uint32_t, uint32_t>> ss_ranges;
  // the per-site histograms as they stood at submission (p == nullptr: off). A merged launch splits ss_ranges into the members
  // submitted with the histograms on (sh_ranges) and the others (ss_plain_ranges)
  dyneng::SiteHist ss_hist;
  std::vector<std::pair<uint32_t, uint32_t>> sh_ranges, ss_plain_ranges;
  dyneng::DevBuf d_bm;                         // [3][n] uint32 low / high / edge_rows (band_margin_kernels.hpp), when asked for
  bool bm_ready = false;                       // the last job computed the margins into d_bm
  dyneng::PinnedBuf h_descs, h_state, h_rows;  // h_state/h_rows: D2H targets of the asynchronous path
  dyneng::PinnedBuf h_stats;                   // wave-cycle statistics of the read-queue launch
  dyneng::PinnedBuf h_sig;                     // staging of pageable caller signals (asynchronous path)
  // raw asynchronous path: [offsets | shift | scale | raw samples] staged in h_sig; device-side scratch of the preprocessing
  dyneng::DevBuf d_norm, d_meta;
  uint64_t n_wide = 0;          // reads of this batch that take the banded-lattice kernel for their half band
  dyneng::DevBuf d_arena;       // band_reads.hip (wide reads, or every read of a guided batch): queue head + one lattice arena per workgroup
  // guided band (dyn_batch_set_guide): every ok read of a guided batch takes the banded-lattice kernel, inside a window
  // of half width guide_hw around its guide (align jobs, and the train job through dyn_batch_train_guided alone); a synchronous
  // batch only, so it never joins a session or a merged launch
  bool guided = false;
  uint32_t guide_hw = 0;
  dyneng::DevBuf d_guide;       // [samples of the batch] int32 centres (HostRead::sig_off counts from here)
  // guide refinement (dyn_batch_set_guide_refine): the next guided align(calc = 1) runs up to guide_refine alignments per read,
  // each inside the path the one before called, until a read's guide reproduces itself
  uint32_t guide_refine = 1;
  dyneng::DevBuf d_gref;        // uint32 [n] rounds | [n] converged | [64] the two list lengths | [n] | [n] the two lists of reads
  bool gref_ready = false;      // the last job refined: d_gref holds rounds / converged
  // the self-guided band of a TICKET (want.auto_guide_hw, 0: a plain ticket). Such a ticket runs alone -- never merged, never
  // published into a resident session: the front thread makes its guide on the compute stream (enqueue_auto_guide) and enqueue_job
  // aligns it as a guided batch, every read refined inside ONE launch (band_reads.hpp, BandArgs::refine_rounds)
  dyneng::PinnedBuf h_gdescs;   // the guide pre-pass's descriptor table (enqueue_job fills h_descs while that copy may be pending)
  dyneng::PinnedBuf h_gref;     // a ticket's rounds | converged, copied out with its state
  uint64_t arena_bytes = 0;     // what the last job asked of d_arena beyond the queue head: every workgroup's lattice arena
  // the guide rescue (want.rescue_hw, 0: off; guide_rescue_kernels.hpp). Such a job is a classic launch -- a ticket is never merged,
  // never published into a resident session
  // uint32 [n] rounds | [n] converged | uint8 [n] code (padded to 256 B) | uint32 [64] list length | [n] list | [3 n] margins
  // (when the batch did not ask for them itself)
  dyneng::DevBuf d_resc;
  dyneng::DevBuf d_resc_st, d_resc_pp, d_resc_pathn, d_resc_segrow;  // the rescue alignment's own state / path rows / segment rows
  dyneng::PinnedBuf h_resc;     // a ticket's rounds | converged | code, copied out with its state
  bool gr_ready = false;        // the last job ran under the switch: d_resc holds rounds / converged / code
  bool host_only = false;       // created on a handle without a device: the read table alone (validation, no job)
  dyneng::SessionGeom sess_geom;  // session_plan's decision for this ticket (ok = false: none taken)
  bool has_raw = false;
  RawSource raw_src;
  std::vector<hipEvent_t> events;              // before / after the read queue / after the per-segment kernels
  hipEvent_t ev_in = nullptr, ev_done = nullptr, ev_out = nullptr;  // ev_done: every kernel of the last job has finished
  uint32_t n_chunks = 0;                       // launches enqueued by the last job (0 or 1)
  std::vector<uint8_t> strict_flag;            // per read: took the certified sweeps in the last job
  dyn_timing timing{};
  bool aligned = false, trained = false;
  int last_calc = 0;
  // ---- asynchronous submission (async_engine.cpp) ----
  bool async = false;
  DynJob job = DynJob::AlignFull;
  const double* in_signals = nullptr;
  const uint64_t* in_sig_offsets = nullptr;
  const char* in_seqs = nullptr;
  const uint64_t* in_seq_offsets = nullptr;
  dyn_align_out* out_align = nullptr;
  dyn_train_out* out_train = nullptr;
  double* out_pooled = nullptr;
  // dyn_batch_device_pooled computes the device-resident pooled statistics on its first call: what it needs of the launch
  bool pooled_on_device = false;
  int pool_nr = 0;
  uint32_t pool_max_N = 0;
  int rc = DYN_OK;             // result of the pipeline stages
  std::string error;           // message for rc != DYN_OK (copied to the handle by dyn_batch_wait)
  bool done = false;
  // ---- merged launches (async_engine.cpp): tickets that waited together share ONE read-queue launch ----
  // A member ticket owns no device buffers of its own: its reads are reads [g_read0, g_read0 + n) and its segment rows
  // [g_seg0, g_seg0 + capacity) of the group's batch, which lives as long as any member does.
  std::shared_ptr<dyneng::BatchGroup> group;
  uint64_t g_read0 = 0, g_seg0 = 0;
  // merged batches (the group's own batch): no contiguous signal array -- one pointer per read (float64 samples)
  const double* const* in_sig_ptrs = nullptr;
  // ---- a ticket of the resident read queue (Session) ----
  bool in_session = false;
  uint32_t sess_reads = 0;             // reads published (the value its completion word reaches)
  uint32_t sess_waves = 0;
  int sess_blk = 0;                    // the session's control block
  uint64_t sess_gen = 0;               // ... and the session's number (Session::blk_gen)
  int sess_retries = 0;                // times the ticket was published again after its session had aborted
  volatile uint32_t* sess_flag = nullptr;
  dyneng::DevBuf d_tctl;               // the ticket's control block (reads done, wave-cycle statistics)
  uint32_t sess_max_N = 0;
  uint64_t sess_rows_total = 0;
  const int32_t* kmers() const { return h_kmers.as<int32_t>(); }
};

namespace dyneng {

// The batch a merged launch runs, and everything it borrows pointers into: the members' concatenated per-read metadata.
struct BatchGroup {
  dyn_batch* g = nullptr;               // the launch's batch (internal: never handed to a caller)
  std::vector<dyn_batch*> members;      // in submission order; cleared once they are complete
  std::vector<uint64_t> sig_offsets, seq_offsets, vbz_bytes, vbz_read_off, vbz_skip;
  std::vector<uint32_t> vbz_samples;
  std::vector<const void*> ptrs;        // one source pointer per read (raw slices, float64 signals) or per VBZ chunk
  std::vector<double> shift, scale;
  std::vector<float> cal_offset, cal_scale;
  std::string seqs;
  std::vector<uint32_t> site_ids;       // the members' per-base ids, concatenated like seqs (DYN_SITE_NONE for members without)
  ~BatchGroup();
};

}  // namespace dyneng

namespace dynk {
struct BandArgs;  // band_reads.hpp
}

namespace dyneng {

// ---- shared between the engine's translation units (dynamont_mi.cpp, site_table.cpp, launch.cpp, session.cpp, async_engine.cpp) ----
int need_device(dyn_aligner* a);
// CU-masked streams (every CU enabled: a hardware queue of their own) are parked per device and reused, never destroyed
// (dynamont_mi.cpp); nullptr when the runtime provides none. The session stream and a dyn_comm's stream come from here.
hipStream_t take_masked_stream(int device, int n_cus);
void park_masked_stream(int device, hipStream_t s);
// per-batch buffers come from / go back to the handle's BufCache
void attach_cache(dyn_batch* b);
// validateInput + sequenceToKmers of every read; fills b->reads / b->h_kmers / capacity / max_T / max_N
// (pinned: k-mer codes go to pinned memory for an asynchronous H2D; false = plain malloc, no HIP call)
// site_ids: the caller's per-base site ids, packed like seqs (pinned batches only): b->h_sites gets the per-row ids beside the codes
int host_prepare(dyn_batch* b, const dynhost::PoreModel& m, bool pinned, uint64_t n_reads,
                 const uint64_t* sig_offsets, const char* seqs, const uint64_t* seq_offsets, HelperPool* pool,
                 const uint32_t* site_ids = nullptr);
// what dyn_aligner_stage_site_ids left for the batch-creating call `api` whose sequences span seq_offsets[0 .. n]: consumed here
// whatever the outcome. *ids = nullptr: nothing was staged. DYN_ERR_INVALID_ARGUMENT (text in last_error): the count differs.
int take_staged_sites(dyn_aligner* a, const char* api, uint64_t n_reads, const uint64_t* seq_offsets, const uint32_t** ids);
// allocate the per-batch device buffers (from the handle's cache)
int alloc_batch_buffers(dyn_batch* b, uint64_t total_sig);
// enqueue every kernel of `job` on the handle's compute stream without synchronising the host
int enqueue_job(dyn_batch* b, DynJob job);
// the guide pre-pass of dyn_batch_auto_guide / of a ticket under dyn_aligner_set_auto_guide, on the compute stream behind the
// batch's preprocessing: d_guide zero-filled, the descriptor table (longest read first, in the batch's pinned h_gdescs),
// launch_auto_guide. Marks the batch guided at half_width; does not wait. Caller holds a->mu, the session is quiesced.
int enqueue_auto_guide(dyn_batch* b, uint32_t half_width);
// ---- resident read queue (session.cpp); all under a->mu ----
// could this ticket run in a session at all? (before host_prepare: kind and size only)
bool session_candidate(const dyn_batch* b);
// After host_prepare: will the ticket be published into a session (the open one, or one opened for it)? Closes an open
// session that cannot take it. *use = false: the classic launch (the caller quiesces the session first).
int session_plan(dyn_batch* b, bool* use);
// descriptors, per-read state, control block -> copy-in stream; the ticket's record published behind them (opens the
// session first if none is open). The ticket's inputs must already be enqueued on the copy-in stream.
int session_publish(dyn_batch* b);
// The ticket's session is gone (its waves left at the idle watchdog) and the ticket is incomplete: wait until that session's
// kernel has ended, then publish the ticket again -- into the session that is open now if it fits, else into a new one.
// All of its reads are redone (the results of those that had finished are the same). *republished = false: nothing was
// missing after all (the waves that were still busy finished the ticket before they left). Caller holds a->mu.
int session_recover(dyn_batch* b, bool* republished);
// what launch_segments and launch_kmer_summary get for this batch's align(calc = 1) job: one entry per range of reads whose
// ticket asked for the summary (empty: none did)
std::vector<dynk::KmerSummary> kmer_summary_args(const dyn_batch* b);
// the same for the per-site summary (empty: none asked, or none of those that asked staged ids)
std::vector<dynk::SiteSummary> site_summary_args(const dyn_batch* b);
// the same for the site calls (b->out[OUT_SITE_CALLS] must be ready; empty: not asked for). A batch without ids, or a merged launch's
// members without, get the NaN columns: one entry with sites == nullptr covers them
std::vector<dynk::SiteCalls> site_call_args(const dyn_batch* b);
// the same for the band margins (b->d_bm must hold 3 * n uint32: band_margin_prepare)
std::vector<dynk::BandMargin> band_margin_args(const dyn_batch* b);
// ---- the launch path's shared steps (launch.cpp; the host-only rules behind them: launch_plan.hpp) ----
// the batch's pinned initial per-read state: the host-side status (ntk: DYN_READ_NTK_MISMATCH for every ok read), everything else 0
dynk::ReadState* init_read_state(dyn_batch* b, bool ntk);
// bytes the lattice arenas in `buf` may take: 0.8 of what is free, what `buf` holds and what is parked, within the budget if asked
int arena_room(dyn_aligner* a, const DevBuf& buf, bool cap_by_budget, uint64_t* room);
// `buf` holds `want` bytes afterwards: parked pools are given back first when memory is tight, and the compute stream is waited
// for when the buffer that grows is the handle's (the ticket before may still be working in it)
int grow_arena(dyn_aligner* a, DevBuf& buf, uint64_t want);
// launch_band_reads' arguments as far as the queue's `q` and the arenas in arena_buf (256-byte head, then arena_bytes per
// workgroup) decide them: descs, sig, par, st, tb, head, arena, exp_tab, m1, e2, z_fail_status
dynk::BandArgs band_args_common(const dyn_batch* b, const dynk::QueueArgs& q, int z_fail, const DevBuf& arena_buf, uint64_t arena_bytes);
// which band margins the rider tail takes: the diagonal's (the first range rides in launch_segments), a guided batch's against its
// guide window, or none -- the guide rescue's stage has taken them
enum class Margins { Diagonal, Guided, Taken };
// launch_segments with the level / score columns, the per-k-mer and per-site summaries and the margins of an align(calc = 1) job or
// ticket on `s`; the caller has prepared (and zeroed) OUT_LEVELS / OUT_SCORES and the margins' room
void enqueue_riders(dyn_batch* b, const dynk::ReadDesc* descs, int n, uint64_t rows_total, uint32_t max_N, const dynk::ReadState* st,
                    const dynk::TraceBuffers& tb, hipStream_t s, Margins margins);
// what the batch remembers of the job just enqueued: tm (with reads_ok / reads_strict filled in), the strict flags, n_chunks,
// aligned / trained / last_calc
void record_job(dyn_batch* b, dyn_timing tm, DynJob job, bool calc, uint64_t reads_ok, uint64_t n_strict, const std::vector<uint32_t>& strict_rows,
                uint32_t n_chunks);
// bm_ready and the room for the margins of an align(calc = 1) job of this batch / ticket
int band_margin_prepare(dyn_batch* b, bool calc);
// What a job of kind `job` submitted NOW through `api` ("dyn_batch_align", "dyn_batch_align_async": `ticket`) takes of the handle's
// switches: the five that concern align(calc = 1) jobs outside modes ntk / resquiggle alone are masked (guide rescue, auto-guide
// -- tickets only --, posterior samples, border interval, soft levels), and a combination the rule table (dynamont_mi.cpp) or a guided batch
// forbids is refused with its text in last_error. No HIP call, no lock but err_mu: the same answer with and without a device.
int resolve_job_options(dyn_aligner* a, DynJob job, bool ticket, bool guided, const char* api, JobOptions* out);
// what the job's switches ask of output k: 0 = nothing, else what OutputBuf::ready becomes (1; OUT_SAMPLES: the count)
int output_wanted(const JobOptions& w, Output k);
// room for output k of this job and ready = `ready` (0: the output is off); then its zeroing on `s` -- the rows of reads that fail
// keep the zeros. output_prepare does both (classic launches); a session ticket ensures at publish and zeroes at finish.
int output_ensure(dyn_batch* b, Output k, int ready);
int output_zero(dyn_batch* b, Output k, hipStream_t s);
int output_prepare(dyn_batch* b, Output k, int ready, hipStream_t s);
// the per-segment kernels and the statistics copy of a COMPLETED session ticket, on `s`
int session_finish_enqueue(dyn_batch* b, hipStream_t s);
int session_collect_timing(dyn_batch* b);
// no ticket will follow: the resident waves leave once what is published is done (returns at once)
int session_close(dyn_aligner* a);
// close, wait until the kernel has left, collect its statistics: the lattice pool is free for a classic launch afterwards
int session_quiesce(dyn_aligner* a);
// after the compute stream has passed the batch: read the event timings into b->timing
int collect_timing(dyn_batch* b);
// rows/state (host copies) -> the caller's columns; reads [read0, read0 + n) of b, whose segment rows start at seg0, land at
// index 0 of `out` (a member of a merged launch; the whole batch: read0 = seg0 = 0, n = b->n)
void unpack_align(const dyn_batch* b, const dynk::ReadState* st, const dynk::SegRow* rows, dyn_align_out* out,
                  HelperPool* pool, uint64_t read0 = 0, uint64_t n = ~0ull, uint64_t seg0 = 0);
// host finalisation of runTraining / trainTransition from host copies of the per-column sums
void finalise_train(const dyn_batch* b, const dynk::ReadState* st, const double* cw, const double* c1,
                    const double* c2, const double* tr, dyn_train_out* out, double* pooled3n);

struct Pipeline {
  explicit Pipeline(dyn_aligner* a);
  ~Pipeline();
  void submit(dyn_batch* b);
  int wait(dyn_batch* b);
  void drain();

  // one read-queue launch on its way through the stages: a ticket on its own, or a group of tickets merged into one batch
  struct Work {
    dyn_batch* b = nullptr;                  // the batch that runs (the ticket itself, or the group's batch)
    std::shared_ptr<BatchGroup> grp;         // set for merged launches
    int rc = DYN_OK;
  };

  dyn_aligner* a;
  HelperPool helpers;
  std::thread t_front, t_back;
  std::mutex m;
  std::condition_variable cv_front, cv_back, cv_done;
  std::deque<dyn_batch*> q_front;
  std::deque<Work> q_back;
  uint64_t in_flight = 0;        // tickets submitted and not yet done
  uint64_t peak_in_flight = 0;   // the most the caller has kept in flight: bounds the tickets one launch takes
  uint64_t launches_pending = 0; // launches handed to the GPU whose results have not been unpacked yet
  bool stop = false;

 private:
  void front_loop();
  void back_loop();
  int front_stage(dyn_batch* b);
  int back_stage(dyn_batch* b, const std::shared_ptr<BatchGroup>& grp);
  int wait_resident(dyn_batch* b);
  void close_idle_session();
  std::shared_ptr<BatchGroup> merge(const std::vector<dyn_batch*>& tickets);
};

}  // namespace dyneng
