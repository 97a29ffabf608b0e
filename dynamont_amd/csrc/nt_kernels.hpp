// nt_kernels.hpp -- device-side data layout and launch interface of the NT hot path.
#pragma once

#include <cstddef>
#include <cstdint>

#include <hip/hip_runtime.h>

#include "dp_math.hpp"
#include "lattice_phase.hpp"

namespace dynk {

using dynmath::Emis;

// One 64-lane wavefront owns one read. A lattice row has at most 2*bw+1 in-band cells
// (NT_aligner_api.cpp:90-108); they live in P = 64*CPL "band slots", slot = n mod P, so a
// lattice column keeps its lane and register for as long as it is in the band and the band
// shift of the reference (mShift/eShift, NT_aligner_api.cpp:131-138) never moves data.
// P must exceed the band width by one so the out-of-band neighbour of an edge cell is a real
// (always -inf) slot and never aliases an in-band cell.
constexpr int CPL = 7;                       // cells per lane
constexpr int P = 64 * CPL;                  // 448 slots per row
constexpr int MAX_HALF_BAND = (P - 2) / 2;   // 2*bw+1 <= P-1  ->  bw <= 223 (band <= 447)
// 64-bit words of a row's record in PagePool::bits: 64 bytes per row, one BYTE per lane of the forward sweep -- the lane's CPL
// decision bits and, in bit 7, whether its float LPE cells of the row were stored (decision_record.hpp, lpe_liveness.hpp;
// in-place layout: set in every lane).
constexpr int ROW_WORDS = CPL + 1;

// The lattice of a read lives in PAGES of 2^log_rows rows taken from a pool that all reads of a
// launch share: a read holds ceil((T+1) / rows_per_page) pages from the moment a wave starts its
// backward sweep until its traceback is done. A wave keeps the page numbers of its current read in
// LDS (PT_MAX entries), so rows_per_page is chosen per launch such that the longest read fits.
constexpr int PT_MAX = 512;
// Waves per SIMD of the read queue (an experiment switch: 2 = eight waves per CU, a 2-deep row ring)
#ifndef DYN_WAVES_PER_SIMD
#define DYN_WAVES_PER_SIMD 1
#endif
constexpr int WAVES_PER_CU = 4 * DYN_WAVES_PER_SIMD;
constexpr uint32_t NO_PAGE = 0xffffffffu;

struct ReadDesc {
  uint64_t sig_off;   // first sample in the signal pool (doubles)
  uint64_t par_off;   // first entry in the per-column emission table; entry n-1 <-> column n
  uint64_t path_off;  // per-row path arrays [T]
  uint64_t seg_off;   // first output row of this read
  uint32_t T;         // signal length + 1   (NT_aligner_api.cpp:241)
  uint32_t N;         // k-mer count + 1     (NT_aligner_api.cpp:242)
  uint32_t bw;        // min(band/2, N/2)    (NT_aligner_api.cpp:243)
  uint32_t read;      // index into the per-read state arrays
  double ratio;       // double(N)/double(T) (NT_aligner_api.cpp:96)
  uint32_t first_page;  // pages first_page .. first_page+n_pages-1 were reserved by the host (first round of a
                        // launch), or NO_PAGE: the wave takes n_pages from the pool's free list
  uint32_t n_pages;     // lattice rows 0..T in pages; 0 for jobs without a stored lattice
  uint32_t flags;       // READ_STRICT / READ_STRICT_START: this read takes the bit-for-bit sweeps (dp_math_strict.hpp)
  uint32_t strict_rows; // READ_STRICT_START: forward rows 1 .. strict_rows in the strict arithmetic
};
constexpr uint32_t READ_STRICT = 1u;        // every row of both sweeps
constexpr uint32_t READ_STRICT_START = 2u;  // the backward sweep and the first strict_rows rows of the forward sweep

struct ReadState {
  double Zb;          // backwardE(0,0)          (NT_aligner_api.cpp:286)
  double Zf;          // forwardE(T-1, mid(T-1)) (NT_aligner_api.cpp:285)
  int32_t status;     // dyn_read_status
  uint32_t n_segments;
};

struct SegRow {
  uint32_t signal_pos;
  uint32_t sequence_pos;
  double probability;
};

struct TraceBuffers {
  double* pp;         // [path] posterior of the path cell of each row
  uint32_t* pathn;    // [path] lattice column of the path cell (bit 31: state M)
  uint32_t* segrow;   // [segments] row of each segment's M cell
  double* med_hi;     // [segments] upper middle order statistic
  double* med_lo;     // [segments] lower middle order statistic (even counts)
};

struct TrainBuffers {
  double* col_w;      // [par] expected count per lattice column
  double* col_s1;     // [par] sum gamma*x
  double* col_s2;     // [par] sum gamma*x^2
  double* trans;      // [2*reads] expected E->M and E->E transition counts (linear domain)
};

// Page pool + read queue of one launch (device pointers).
struct PagePool {
  double* ws;           // [n_pages][rows_per_page][P]   backward-E (8 B per slot); in place: (float LPM, float LPE)
  float* lpe;           // [n_pages][rows_per_page][P]   float LPE per slot (separate layout) or nullptr
  uint64_t* bits;       // [n_pages][rows_per_page][ROW_WORDS] the rows' records: a byte per lane, its decision bits and "LPE stored"
  uint32_t* free_list;  // stack of free page numbers
  // ctl (32-bit words): [0] lock of the free-page stack, [1] queue head (next read), [2] free pages on the
  // stack, [3] abort (a wave gave up waiting: the queue drains, the host reports the launch as failed),
  // [4] reads whose pages are in place, [5] waves waiting for pages.
  // ctl + QUEUE_STATS (64-bit words): wave-cycles spent in backward, forward, traceback, waiting for pages,
  // lifetime (all summed over the waves of the launch), longest lifetime; then the strict reads apart: their backward and
  // forward wave-cycles, registers recomputed by the certified logPlus' fallback, rows run in the certified arithmetic.
  uint32_t* ctl;
  int log_rows;         // rows per page = 1 << log_rows
  uint32_t n_pages;
  uint32_t reserve_after;  // waits (x ~30 us) after which a wave RESERVES its request for pages; 0 = never (one launch per batch:
                           // the queue is finite and its order planned). Paged sessions: 64
};
constexpr int QUEUE_CTL_WORDS = 32;   // 32-bit words reserved for ctl (stats start at word 8, 8-byte aligned)
constexpr int QUEUE_STATS = 8;        // first stats word (as uint32 index)
constexpr int QUEUE_N_STATS = 10;

enum QueueJob { JOB_Z = 0, JOB_ALIGN = 1, JOB_ALIGN_INPLACE = 2, JOB_TRAIN = 3, JOB_TRAIN_ZCHECK = 4 };
// On top of JOB_ALIGN / JOB_ALIGN_INPLACE, k_read_queue's template argument carries the launch's lattice phases: the bits JOB_BORDER,
// JOB_SAMPLE, JOB_INTERVAL and JOB_SOFT, and lattice_phases(), the one place that decides which of them a launch carries
// (lattice_phase.hpp).

// posterior path samples (dyn_aligner_set_posterior_samples; sample_kernels.hpp). count == 0: not asked for (and the launch is
// the one it has always been). The per-read counts of dead samples live behind the planes: start + count * capacity, one per
// read of the batch.
struct SampleOut {
  uint32_t* start;    // [count][capacity] segment starts, sample-major, then [reads of the batch] dead samples; zeroed by the caller
  uint64_t capacity;  // the batch's segment capacity: the stride between two samples' planes
  uint64_t seed;
  int count;          // K, 1 .. 64
};

// per-border credible intervals (dyn_aligner_set_border_interval; interval_kernels.hpp): the four columns of a launch, in ONE buffer of 24 bytes per output row:
//   double mean[capacity] | double sd[capacity] | uint32 lo[capacity] | uint32 hi[capacity]       (zeroed by the caller)
// tail == 0: not asked for. It shares the train buffers' / the samples' place in QueueArgs and BandArgs: `none` lies on
// SampleOut::count and stays 0, which is how lattice_phases() tells the two apart.
struct IntervalOut {
  double* mean;
  uint64_t capacity;
  double tail;  // a = (1 - mass) / 2, formed by the host
  int none;     // = SampleOut::count: 0
};
static_assert(offsetof(IntervalOut, none) == offsetof(SampleOut, count), "an interval launch reads as a launch without samples");

// posterior-weighted per-base sums (dyn_aligner_set_soft_levels; soft_level_kernels.hpp): the three columns of a launch, in ONE
// buffer of 24 bytes per output row:
//   double weight[capacity] | double sum[capacity] | double sumsq[capacity]                         (zeroed by the caller)
// It shares the same place. `zero` lies on SampleOut::seed / IntervalOut::tail and stays 0 (no interval launch), `tag` lies on
// SampleOut::count / IntervalOut::none and is SOFT_TAG (lattice_phase.hpp), a value neither of the others ever holds.
struct SoftOut {
  double* weight;
  uint64_t capacity;
  uint64_t zero;  // = IntervalOut::tail: 0.0
  int tag;        // = SampleOut::count: SOFT_TAG when asked for
};
static_assert(offsetof(SoftOut, tag) == offsetof(SampleOut, count) && offsetof(SoftOut, zero) == offsetof(IntervalOut, tail),
              "a soft-level launch reads as one without samples and without intervals");

struct QueueArgs {
  const ReadDesc* descs;   // in processing order
  int n_reads;
  int n_static;            // reads [0, n_static) are pre-assigned: wave slot s starts with read s (no queue access)
  const double* sig;
  const Emis* par;
  PagePool pool;
  ReadState* st;
  TraceBuffers tb;
  // A train job has no path to sample and an align job no train buffers: the two share their place, so that the kernel-argument
  // layout of every launch stays what it was before there were samples. All zero (what `QueueArgs q{}` leaves): neither.
  union {
    TrainBuffers tr;    // JOB_TRAIN / JOB_TRAIN_ZCHECK
    SampleOut sample;   // JOB_ALIGN / JOB_ALIGN_INPLACE: posterior path samples, count > 0 when asked for
    IntervalOut interval;  // JOB_ALIGN / JOB_ALIGN_INPLACE: per-border credible intervals, tail > 0 (and sample.count == 0) when asked for
    SoftOut soft;       // JOB_ALIGN / JOB_ALIGN_INPLACE: posterior-weighted per-base sums, tag == SOFT_TAG when asked for
    // Which member an align launch carries is read from ONE word, sample.count (= interval.none = soft.tag), and
    // interval.tail, by lattice_phases() (lattice_phase.hpp) and by nobody else.
  };
  double m1, e2;          // log transition probabilities (NT_aligner_api.cpp:84-86)
  const dynmath::SoftplusNode* sp_tab;
  int z_fail_status;
  // the forward sweep stores the float LPE of a lane group only where a cell has !(LPE < lpe_floor) (lpe_liveness.hpp);
  // lpe_dense: every group is stored. Launches whose border-confidence phase reads whole windows of LPE are dense anyway.
  float lpe_floor = -750.0f;
  int lpe_dense = 0;
  // per-border posterior confidence (dyn_aligner_set_border_confidence): columns indexed like the output rows, zeroed by the
  // caller; border_window == 0: not asked for (and the launch is the one it has always been)
  int border_window = 0;             // W, 1 .. 256
  double* border_p = nullptr;
  double* border_window_p = nullptr;
};
static_assert(sizeof(SampleOut) <= sizeof(TrainBuffers), "the samples take the train buffers' place in QueueArgs / BandArgs");
static_assert(sizeof(IntervalOut) <= sizeof(TrainBuffers), "the intervals take the train buffers' place in QueueArgs / BandArgs");
static_assert(sizeof(SoftOut) <= sizeof(TrainBuffers), "the soft levels take the train buffers' place in QueueArgs / BandArgs");

// ---- the RESIDENT read queue (round 5) ---------------------------------------------------------------------------
// k_read_queue drains ONE batch per launch: its waves finish up to one read apart, and the next launch -- queued on the same
// stream -- waits for the last of them (wave occupancy 0.89-0.91 at 2-3 batches per launch). k_session keeps the waves
// RESIDENT: the host publishes batch after batch ("tickets") into a ring while the kernel runs, a wave that has finished a
// read takes the next one of whatever ticket is next, and the kernel leaves only when the host closes the session (nothing
// left in its pipeline). Tickets complete one by one (a counter per ticket; the wave whose read completes it raises a word
// in pinned host memory), their per-segment kernels and copies run beside the resident waves on other streams.
//  * every wave owns a STATIC arena of `arena_pages` lattice pages (page numbers slot * arena_pages + k): no free list, no
//    lock; the host only opens a session when the pool holds an arena for every wave (separate LPE layout);
//  * inputs of a ticket (descriptors, samples, per-column parameters) were written by H2D copies and small kernels of other
//    streams WHILE this kernel runs, into buffers that earlier tickets used: a wave starts every read with s_dcache_inv and
//    an agent-scope acquire (this CU's L1), and it reads them through ONE `const __restrict__` kernel parameter (in_base +
//    a byte offset from the ticket record), so that wave-uniform loads stay scalar loads (see k_read_queue);
//  * what a wave wrote for a read (state, path arrays) is released (agent scope) before the ticket's counter moves;
//  * every wait is bounded: a wave that has found nothing to do for `idle_limit_ticks` raises the abort word and leaves.
// Validated in isolation by tools/ubench/resident_probe.hip (co-scheduling of the small kernels beside a resident kernel of
// this footprint, freshness of rewritten buffers, and that the resident kernel needs a hardware queue of its own).
struct SessionTicket {      // 128 bytes in device memory, written once per ticket by k_session_publish
  // Byte offsets, not pointers: an address the kernel forms from one of its own pointer PARAMETERS is known to be global
  // memory (global_load / global_store; a pointer loaded from memory is a generic one: flat_ instructions), and loads
  // through the `const __restrict__` in_base stay scalar loads where the address is wave-uniform.
  int64_t descs_off;        // from in_base: ReadDesc[n_reads] in processing order,
  int64_t sig_off;          //   the ticket's signal pool (ReadDesc::sig_off counts doubles from here),
  int64_t par_off;          //   its per-column emission table (ReadDesc::par_off counts entries from here)
  int64_t st_off;           // from out_base: ReadState[], then the five TraceBuffers arrays
  int64_t pp_off, pathn_off, segrow_off, medhi_off, medlo_off;
  int64_t tctl_off;         // the ticket's control block: [0] reads finished; 64-bit statistics from word SESSION_TSTATS on:
                            //   wave-cycles (shader clock) in backward / forward / traceback, [3] the reads' durations in 10 ns
                            //   ticks (s_memrealtime), [6..9] the certified sweeps apart (as QUEUE_STATS)
  int64_t flag_off;         // a word of pinned host memory: set to n_reads by the wave whose read completes the ticket
  uint32_t n_reads;
  uint32_t base;            // the ticket's reads are global indices [base, base + n_reads)
  int32_t z_fail_status;
  uint32_t pad_[7];
};
static_assert(sizeof(SessionTicket) == 128, "one cache line pair per record");
constexpr int SESSION_TSTATS = 2;        // first statistics word of a ticket's control block (as uint32 index, 8-byte aligned)
constexpr int SESSION_TCTL_WORDS = 32;
// session control words (device memory, 32-bit): next global read index, tickets published, closed, abort; 64-bit statistics
// from word SESSION_STATS on: wave-cycles busy (claim to release), idle, lifetime, longest lifetime, reads done, [5] the part
// of idle spent getting pages (paged sessions), [6] idle before a wave's first read (part of idle), [7] a wave's last turn (no read
// left to claim; NOT part of idle: lifetime - busy - idle), [8] the pages part of [6], [9] sum of ([7] >> 10)^2, [10] max of [7], [11] / [12] the read that ended last (k_session)
constexpr int S_HEAD = 0, S_TAIL = 1, S_CLOSED = 2, S_ABORT = 3, SESSION_STATS = 8, SESSION_CTL_WORDS = 40;

struct SessionArgs {
  const SessionTicket* ring;   // [ring_size]; slot i holds ticket i of the session (never reused within one)
  uint32_t ring_size;
  uint32_t arena_pages;        // pages per wave (layout 0)
  uint32_t give_always;        // paged layouts, experiments (DYN_SESSION_GIVE_ALWAYS): surplus pages go back at every read
  uint32_t* ctl;
  PagePool pool;               // ws, lpe, bits, log_rows; layouts 1 / 2 (paged): free_list and ctl as well (k_pool_init first)
  double m1, e2;
  uint64_t idle_limit_ticks;   // s_memrealtime ticks (100 MHz)
  float lpe_floor = -750.0f;   // as QueueArgs
  int lpe_dense = 0;
};

// n_cus workgroups of four waves on `s` -- which must own its hardware queue (hipExtStreamCreateWithCUMask)
// with_strict: the variant that carries the certified sweeps. layout: 0 = an arena per wave (separate LPE), 1 = pages shared
// through the pool's free list (separate LPE), 2 = shared pages, posteriors in place (page-starved batches)
void launch_session(bool with_strict, int layout, const SessionArgs& a, const void* in_base, void* out_base, const dynmath::SoftplusNode* sp_tab,
                    int n_cus, hipStream_t s);
// record `tk` as ticket `index` and make it visible (tail = index + 1); closed: no ticket will follow
void launch_session_publish(SessionTicket* ring, uint32_t* ctl, const SessionTicket& tk, uint32_t index, uint32_t ring_size, hipStream_t s);
void launch_session_close(uint32_t* ctl, hipStream_t s);

// ---- any band (band_reads.hpp): reads whose half band exceeds MAX_HALF_BAND take a generic kernel, one workgroup per read ----
constexpr int WIDE_MAX_B = 4096;                          // band columns per row incl. the two guards (2 bw + 3), held in LDS
constexpr int WIDE_MAX_HALF_BAND = (WIDE_MAX_B - 3) / 2;  // 2 046: band <= 4 093

// P1/P2 on the device: out[i] = hampel((REAL(raw[i]) - shift) / scale); REAL = float when compute_f32.
// raw_dtype: 0 float32, 1 int16, 2 float64, 3 int16 ADC with per-read float32 calibration (pA = (adc + cal_offset) *
// cal_scale in float32; cal_* may be null otherwise). norm_tmp: scratch of total samples * sizeof(REAL).
void launch_preprocess(const void* raw, int raw_dtype, int compute_f32, const uint64_t* offs,
                       const double* shift, const double* scale, const float* cal_offset, const float* cal_scale,
                       void* norm_tmp, double* out, int n_reads, uint64_t max_len, int W, double n_sigmas, hipStream_t s);
void launch_prep_params(const int32_t* kmers, const Emis* model, Emis* par, uint64_t total, uint32_t num_kmers,
                        hipStream_t s);
// free list = pages [first_free, n_pages); queue head = n_static; statistics cleared
void launch_pool_init(const PagePool& pool, uint32_t first_free, int n_static, hipStream_t s);
// The whole per-read pipeline as ONE launch of persistent waves (see nt_kernels.hip): each wave takes
// reads off the queue until it is empty; per read backward -> forward (+ posterior, Viterbi fill,
// decision bits | training statistics) -> Z check -> traceback -> segment-start posteriors.
// n_cus: compute units of the device (one 4-wave workgroup per CU).
// with_strict: the launch holds reads flagged READ_STRICT (JOB_ALIGN / JOB_ALIGN_INPLACE only): the kernel variant
// that carries both arithmetic flavours and branches per read
// Returns what the launch reported. hipErrorInvalidValue, and no launch: no kernel exists for the job with its phases and
// with_strict (a strict launch of a job other than the two align jobs)
hipError_t launch_read_queue(QueueJob job, bool with_strict, const QueueArgs& q, int n_cus, hipStream_t s);
// per-segment signal levels (event_stats.hip): columns indexed like the output rows; mean == nullptr: not asked for
struct EventCols {
  const double* sig;  // the signal the read queue aligned (ReadDesc::sig_off counts from here)
  double* mean;
  double* stdev;
  double* median;
};
void launch_event_stats(const ReadDesc* descs, int n_reads, uint64_t rows_total, const ReadState* st, const TraceBuffers& tb,
                        const EventCols& ev, hipStream_t s);
// per-k-mer level summary of a run (kmer_summary.hip, dyn_aligner_set_kmer_summary); acc == nullptr: not asked for
struct KmerSummary {
  const double* sig;          // the signal the read queue aligned (ReadDesc::sig_off counts from here)
  const int32_t* kmers;       // k-mer code of every lattice column (ReadDesc::par_off counts from here): row j <-> entry j
  unsigned long long* acc;    // the handle's accumulator: [num_kmers][6] n_segments, n_samples, q1 lo / hi, q2 lo / hi
  unsigned long long* totals; // [4] reads_ok, segments, samples, skipped_segments
  uint32_t num_kmers;
  uint32_t read_lo, read_hi;  // the reads [read_lo, read_hi) (ReadDesc::read) contribute: the members of a merged launch
                              // whose handle had the switch on when they were submitted
};
void launch_kmer_summary(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                         const KmerSummary& ks, hipStream_t s);
// per-site level summary of a run (site_summary.hip, dyn_aligner_set_site_summary); acc == nullptr: not asked for
constexpr int SS_FIELDS = 7;  // per site: n_rows, n_samples, dwell_sq, m1_lo, m1_hi, m2_lo, m2_hi
constexpr int SS_TOTALS = 5;  // reads_ok, rows_added, samples_added, rows_without_site, rows_skipped
constexpr int SM_STATS = 3;   // of a sparse table's map (site_map.hpp), behind the totals: n_keys, rows_dropped, sites_dropped
constexpr int SM_N_KEYS = 0, SM_ROWS_DROPPED = 1, SM_SITES_DROPPED = 2;
struct SiteSummary {
  const double* sig;          // the signal the read queue aligned (ReadDesc::sig_off counts from here)
  const uint32_t* sites;      // site id of every output row (ReadDesc::par_off counts from here): row j <-> entry j
  unsigned long long* acc;    // the handle's table: [num_sites][7] n_rows, n_samples, dwell_sq, m1 lo / hi, m2 lo / hi
  unsigned long long* totals; // [5] reads_ok, rows_added, samples_added, rows_without_site, rows_skipped
  uint32_t num_sites;
  uint32_t read_lo, read_hi;  // the reads [read_lo, read_hi) (ReadDesc::read) contribute: the members of a merged launch
                              // that asked and staged ids
  // the per-site histograms (dyn_aligner_set_site_histogram); hist == nullptr: off. An aggregate initialiser that stops at
  // read_hi leaves them zero.
  unsigned int* hist;         // [num_sites][bins + 2 + 16] under, level bins 1 .. bins, over, dwell bins 0 .. 15
  uint32_t bins;
  double hist_lo, inv_w;      // level bin of m: u = (m - hist_lo) * inv_w, inv_w = bins / (hi - lo)
  // the sparse mode (dyn_aligner_set_site_summary_sparse, site_map.hpp); map_keys == nullptr: dense, the id is the row. Sparse:
  // acc and hist have `capacity` rows and a row's bucket is looked up (or taken) as it is added; num_sites still bounds the ids.
  // An aggregate initialiser that stops earlier leaves them zero.
  uint32_t* map_keys;         // [capacity], 0xFFFFFFFF: empty
  uint32_t capacity;
  unsigned long long* map_stats;  // [3] n_keys, rows_dropped, sites_dropped
};
void launch_site_summary(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                         const SiteSummary& ss, hipStream_t s);
constexpr int SH_DWELL_BINS = 16;
constexpr int SH_BINS_MAX = 254;
constexpr int SQ_PROBS_MAX = 8;
constexpr uint32_t SQ_NO_BIN = 0xFFFFFFFFu;
// quantiles of a window of the per-site level histograms (k_site_quantiles, site_summary_kernels.hpp). out: uint32
// [count] n, then rank, bin, below, in_bin as [count][n_probs] each
struct SiteQuantiles {
  const unsigned int* hist;   // the first site's counters; a site's bins + 2 + 16 counters are contiguous
  uint32_t bins;
  uint32_t count;             // sites of the window
  int n_probs;                // 1 .. 8
  double probs[SQ_PROBS_MAX];
  uint32_t* out;
};
void launch_site_quantiles(const SiteQuantiles& sq, hipStream_t s);
constexpr uint32_t SC_NO_AT = 0xFFFFFFFFu;
constexpr int SC_PAIR_BYTES = 2 * 8 + 6 * 4;
// two windows of the per-site histograms compared pair by pair (k_site_compare, site_compare_kernels.hpp). out, SC_PAIR_BYTES per
// pair: uint64 [count] level_num, dwell_num, then uint32 [count] n_a, n_b, level_at, dwell_at, level_side, dwell_side (the sides
// as int32 bits)
struct SiteCompare {
  const unsigned int* hist_a; // the first site's counters of either window; a site's bins + 2 + 16 counters are contiguous
  const unsigned int* hist_b;
  uint32_t bins;
  uint32_t count;             // pairs of the window
  unsigned long long* out;
};
void launch_site_compare(const SiteCompare& sc, hipStream_t s);
constexpr int SM_PAIR_BYTES = 7 * 8 + 6 * 4;
constexpr uint32_t SM_MAX_ITERS = 1024;
// a two-component mixture fitted to the level counters of every pair of two windows (k_site_mixture, site_mixture_kernels.hpp).
// out, SM_PAIR_BYTES per pair: float64 [count] pi1, mu0, mu1, var0, var1, r_a, r_b, then uint32 [count] n_a, n_b, out_a, out_b,
// iters, status
struct SiteMixture {
  const unsigned int* hist_a; // the first site's counters of either window; a site's bins + 2 + 16 counters are contiguous
  const unsigned int* hist_b; // nullptr: the single-sample form
  const uint64_t* exp_tab;    // dynmath::strict_exp_table on the device
  uint32_t bins;
  uint32_t count;             // pairs of the window
  uint32_t max_iters;         // 1 .. SM_MAX_ITERS
  uint32_t min_n;
  double lo, w;               // the histograms' lower bound and bin width (hi - lo) / bins
  double vfloor;              // (w * w) / 12
  double tol_mu, tol_pi;      // tol * w, tol
  double* out;
};
void launch_site_mixture(const SiteMixture& sm, hipStream_t s);
// host columns added into a window of the table and, optionally, of the counters (k_site_add, site_compare_kernels.hpp)
struct SiteAdd {
  unsigned long long* acc;          // the window's first cell of the table: [count][7]
  unsigned long long* totals;       // the table's [5] totals
  const unsigned long long* cols;   // staged [count][7], the table's own field order
  unsigned int* hist;               // the window's first counter, [count][width]; nullptr: the table alone
  const unsigned int* counters;     // staged [count][width]
  uint32_t count;
  uint32_t width;                   // bins + 2 + 16
  int add_totals;                   // 0: totals_in is not added
  unsigned long long totals_in[SS_TOTALS];
};
void launch_site_add(const SiteAdd& sa, hipStream_t s);
// the window calls of a sparse table (site_map_kernels.hpp). k_site_gather: the ids [lo, lo + count) looked up, their cells copied
// into a dense scratch table (and scratch counters when hist is set); an absent id gets zeros
struct SiteGather {
  const uint32_t* keys;             // [capacity]
  uint32_t capacity;
  const unsigned long long* acc;    // the table: [capacity][7]
  const unsigned int* hist;         // [capacity][width]; nullptr: the table alone
  uint32_t width;                   // bins + 2 + 16
  uint32_t lo, count;               // the window of ids
  unsigned long long* out_acc;      // [count][7]; nullptr: the counters alone
  unsigned int* out_hist;           // [count][width]
};
void launch_site_gather(const SiteGather& sg, hipStream_t s);
// k_site_scatter_add: the add of SiteAdd into the rows of the ids [lo, lo + count); a site with any non-zero word is looked up or
// inserted, an all-zero site inserts nothing, a site without a bucket counts in stats[sites_dropped]
struct SiteScatter {
  uint32_t* keys;
  uint32_t capacity;
  unsigned long long* stats;        // [3] n_keys, rows_dropped, sites_dropped
  unsigned long long* acc;          // the table: [capacity][7]
  unsigned long long* totals;       // the table's [5] totals
  unsigned int* hist;               // [capacity][width]; nullptr: the table alone
  const unsigned long long* cols;   // staged [count][7]
  const unsigned int* counters;     // staged [count][width]
  uint32_t width;
  uint32_t lo, count;
  int add_totals;
  unsigned long long totals_in[SS_TOTALS];
};
void launch_site_scatter_add(const SiteScatter& sc, hipStream_t s);
// k_site_map_windows: every occupied bucket sets bit (key >> shift) of bitmap
struct SiteWindows {
  const uint32_t* keys;
  uint32_t capacity;
  int shift;
  unsigned int* bitmap;             // [ceil(((num_sites - 1) >> shift) + 1, 32)] uint32, zeroed by the caller
};
void launch_site_map_windows(const SiteWindows& sw, hipStream_t s);
// the table by content (site_pack_kernels.hpp). k_site_pack_*: the live rows of the table rows [row_lo, row_lo + count) -- an id
// in [site_lo, site_hi), any cell word or counter non-zero -- as records in ascending row order: a count pass, a scan and a write
constexpr int SPK_CHUNK_ROWS = 64;  // rows per live mask: the scratch of a window is sized from it
struct SitePack {
  const uint32_t* keys;             // [capacity], the row's id; nullptr: the table is dense, the row is the id
  const unsigned long long* acc;    // the table: [rows][7]
  const unsigned int* hist;         // [rows][width]; nullptr: the table alone
  uint32_t width;                   // bins + 2 + 16
  uint32_t row_lo, count;           // the window of rows, count <= 2^20
  uint32_t site_lo, site_hi;        // the filter on the ids
  unsigned long long* mask;         // scratch, [ceil(count / 64)]: the live rows of every chunk of 64
  uint32_t* offset;                 // scratch, [ceil(count / 64)]: the live rows in front of every chunk
  unsigned long long* total;        // [1]: the live rows of the window
  uint64_t cap;                     // records the three arrays below hold (the write pass alone reads these four)
  uint32_t* out_site;               // [cap]
  unsigned long long* out_cells;    // [cap][7]
  unsigned int* out_hist;           // [cap][width]
};
void launch_site_pack(const SitePack& sp, hipStream_t s);        // count and scan: *total
void launch_site_pack_write(const SitePack& sp, hipStream_t s);  // the records, behind them on the same stream
// k_site_merge: `count` records added into the rows of the ids site[i] + offset, duplicates allowed; what k_site_scatter_add adds
// and counts, by key
struct SiteMerge {
  uint32_t* keys;                   // nullptr: the table is dense, the id is the row
  uint32_t capacity;
  unsigned long long* stats;        // [3] n_keys, rows_dropped, sites_dropped (sparse)
  unsigned long long* acc;          // the table: [rows][7]
  unsigned long long* totals;       // the table's [5] totals
  unsigned int* hist;               // [rows][width]; nullptr: the table alone
  const uint32_t* site;             // staged [count]
  const unsigned long long* cells;  // staged [count][7]
  const unsigned int* counters;     // staged [count][width]
  uint32_t width;
  uint32_t count;
  uint64_t offset;                  // added to every id
  uint64_t num_sites;               // the bound of id + offset
  int add_totals;
  unsigned long long totals_in[SS_TOTALS];
};
void launch_site_merge(const SiteMerge& sm, hipStream_t s);
// per-read site calls (site_call_kernels.hpp, dyn_aligner_set_site_calls): every output row scored against the per-site model of
// dyn_aligner_set_site_model; prob == nullptr: not asked for
constexpr int SC_MODEL_FIELDS = 5;  // per table row: pi1, mu0, mu1, var0, var1 (all zero: not set)
struct SiteCalls {
  const double* sig;          // the signal the read queue aligned (ReadDesc::sig_off counts from here)
  const uint32_t* sites;      // site id of every output row (ReadDesc::par_off counts from here); nullptr: none staged, every row the NaN
  const double* model;        // [num_sites][5], sparse [capacity][5]; nullptr: none uploaded, every row the NaN
  const uint32_t* map_keys;   // the map of a sparse table (only ever read); nullptr: dense, the id is the row
  uint32_t capacity;
  uint32_t num_sites;
  uint32_t read_lo, read_hi;  // the reads [read_lo, read_hi) (ReadDesc::read) are written
  const uint64_t* exp_tab;    // dynmath::strict_exp_table on the device
  double* prob;               // the two columns, indexed like the output rows (ReadDesc::seg_off + j)
  double* z;
};
void launch_site_calls(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                       const SiteCalls& sc, hipStream_t s);
// k_site_model_scatter: a staged window of model rows into the rows of the ids [lo, lo + count) of a sparse table; a set row finds
// or inserts its bucket (one without a bucket counts in *dropped), a row that is not set inserts nothing
struct SiteModelScatter {
  uint32_t* keys;
  uint32_t capacity;
  unsigned long long* stats;        // [3] n_keys, rows_dropped, sites_dropped (n_keys moves with an insert)
  double* model;                    // [capacity][5]
  const double* rows;               // staged [count][5]
  uint32_t lo, count;
  unsigned long long* dropped;      // one counter of this call
};
void launch_site_model_scatter(const SiteModelScatter& ms, hipStream_t s);
// k_site_model_gather: the model rows of the ids [lo, lo + count) of a sparse table into a dense scratch; an absent id gets zeros
struct SiteModelGather {
  const uint32_t* keys;
  uint32_t capacity;
  const double* model;              // [capacity][5]
  uint32_t lo, count;
  double* out;                      // [count][5]
};
void launch_site_model_gather(const SiteModelGather& mg, hipStream_t s);
// per-border segment quality scores (segment_scores.hip, dyn_aligner_set_segment_scores): columns indexed like the output
// rows, zeroed by the caller; median_delta == nullptr: not asked for
struct ScoreCols {
  const double* sig;  // the signal the read queue aligned (ReadDesc::sig_off counts from here)
  double* median_delta;
  double* mad_delta;
  double* homogeneity;
  double* scratch;    // one more column: the trimmed median of a row between the two homogeneity launches
  int window;         // W, 1 .. 256
};
void launch_segment_scores(const ReadDesc* descs, int n_reads, uint64_t rows_total, uint32_t max_N, const ReadState* st,
                           const TraceBuffers& tb, const ScoreCols& sc, hipStream_t s);
// band-margin diagnostics (band_margin.hip, dyn_aligner_set_band_margin): three uint32 per read, indexed by ReadDesc::read;
// low == nullptr: not asked for
struct BandMargin {
  uint32_t* low;              // smallest slack of the called path to a real lower band edge (0xFFFFFFFF: never real)
  uint32_t* high;             // ... to a real upper band edge
  uint32_t* edge_rows;        // path rows with a real slack of 0
  uint32_t read_lo, read_hi;  // the reads [read_lo, read_hi) (ReadDesc::read) are initialised and computed: the members of a
                              // merged launch whose handle had the switch on when they were submitted
};
void launch_band_margin(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                        const BandMargin& bm, hipStream_t s);
// per-segment median posterior + output rows for all reads of descs (after launch_read_queue), then the signal levels when
// `ev` asks for them, the per-k-mer summary when `ks` does, the segment scores when `sc` does and the band margins when `bm` does
void launch_segments(const ReadDesc* descs, int n_reads, uint64_t rows_total, uint32_t max_N, const ReadState* st,
                     TraceBuffers tb, SegRow* rows, int kmer_size, hipStream_t s, const EventCols& ev = EventCols{},
                     const KmerSummary& ks = KmerSummary{}, const ScoreCols& sc = ScoreCols{}, const BandMargin& bm = BandMargin{});
// per-read signal rescaling (rescale.hip, dyn_aligner_set_rescale): the transform x = (x0 - A) / B of read `read`
struct RescaleState {
  double A;         // shift: 0.0 until a fit is applied
  double B;         // scale: 1.0 until a fit is applied
  int32_t applied;  // fits applied so far
  int32_t frozen;   // a fit was refused (or the read failed): no later fit
  int32_t fitted;   // the last fit was applied: k_rescale_apply recomputes the read's signal
  int32_t pad;
};
void launch_rescale_init(RescaleState* rs, uint64_t n_reads, hipStream_t s);
// between two passes: the fit of every read of descs (after the read queue and the wide-band kernel of the pass), then
// sig = (sig0 - A) / B for the reads whose fit was applied. y: scratch column indexed like the output rows.
void launch_rescale_pass(const ReadDesc* descs, int n_reads, uint32_t max_T, const ReadState* st, const TraceBuffers& tb,
                         const double* sig0, double* sig, const Emis* par, double* y, RescaleState* rs, hipStream_t s);
// pooled[3*num_kmers] (zeroed by the caller) = per-k-mer (w, s1, s2) of the ok reads in descs, summed in a FIXED order:
// per read over its columns ascending, then over the reads in input order -- bit for bit the host's sum (pool_stats.hip).
// work: pool_stats_work_bytes(total_cols) device bytes; temp: pool_stats_temp_bytes(...) (rocprim's radix sort).
size_t pool_stats_temp_bytes(uint64_t total_cols, uint64_t num_kmers);
size_t pool_stats_work_bytes(uint64_t total_cols);
hipError_t launch_pool_stats(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const int32_t* kmers,
                             TrainBuffers tb, double* pooled, uint64_t num_kmers, uint64_t total_cols, void* work, void* temp,
                             size_t temp_bytes, hipStream_t s);

}  // namespace dynk
