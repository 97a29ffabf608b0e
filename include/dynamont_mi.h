/*
 * dynamont_mi.h -- C ABI of the MI355X-native NT ("basic" mode) resquiggling core.
 *
 * This is the drop-in boundary for the one hot path of rnajena/dynamont that this repository
 * accelerates. The reference has no C ABI of its own: its boundary is the pybind11 class
 * `_dynamont.Aligner` (src/cpp/aligner_bindings.cpp:180-219) over the virtual C++ interface
 * dynamont::Aligner::{align,train} (include/dynamont/aligner.hpp:72-81). Every entry point
 * below names the reference interface it replaces. All citations are relative to the
 * reference checkout.
 *
 * Conventions: plain pointers and sizes only; no exceptions cross the ABI; functions return
 * a dyn_status; message texts equal the reference's exception texts (callers print them
 * into the `.errors` file, segment.py:172-176, so they are observable output).
 * A handle is bound to ONE GPU (one process per GPU; shard reads across handles/ranks, or use
 * dyn_multi_* below, which owns one handle per device). GPU work of one handle is serialised
 * internally, so calls on DIFFERENT batches of one handle may come from different threads; a
 * single batch object must not be used from two threads at once.
 */
#ifndef DYNAMONT_MI_H
#define DYNAMONT_MI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DYN_ABI_VERSION 10 /* 10 (number kept; look the symbol up): guided-band training: dyn_batch_train_guided (additive). 10 (number kept; look the symbols up): guided band: dyn_batch_set_guide, dyn_batch_arena_bytes (additive). 10 (number kept; look the symbols up): band-margin diagnostics: dyn_aligner_set_band_margin, dyn_batch_fetch_band_margin (additive). 10 (number kept): per-k-mer level summary of a run: dyn_aligner_set_kmer_summary, dyn_aligner_kmer_summary_fetch / _reset (additive). 10: per-read signal rescaling: dyn_aligner_set_rescale, dyn_batch_fetch_rescale (additive). 9: per-segment signal levels: dyn_aligner_set_event_stats, dyn_batch_fetch_events, dyn_format_csv[_bound]_events, dyn_csv_sink_open_ex (additive). 8: dyn_aligner_session_idle_split (additive). 7: dyn_aligner_session_page_wait, dyn_comm_gather_bytes / _gathered_bytes / _allreduce_f64 (additive). 7: half bands 224 .. 2 046 are computed (the generic kernel, today band_reads.hip). 5: any band constructs (DYN_READ_BAND_TOO_WIDE per read); dyn_bam_*, dyn_csv_sink_wait / _open_part */

/* device argument of dyn_aligner_create: bind no GPU. Such a handle serves the host-side
 * contract only (model loading, dyn_aligner_info/_model, dyn_validate_batch, and dyn_batch_create[_raw] as far as the
 * read table: validation and k-mer coding, nothing uploaded -- what dyn_batch_set_guide's checks need); every compute
 * entry point (dyn_batch_align / _train, the getters, the asynchronous API) fails with DYN_ERR_DEVICE -- there is no CPU
 * compute path in this library. */
#define DYN_DEVICE_HOST_ONLY (-2)

/* dynamont::PoreType (include/dynamont/aligner.hpp:26-33), same numbering as the pybind enum
 * (aligner_bindings.cpp:184-189). */
enum dyn_pore {
  DYN_PORE_RNA002 = 0,
  DYN_PORE_RNA004 = 1,
  DYN_PORE_DNA_R9 = 2,
  DYN_PORE_DNA_R10_260 = 3,
  DYN_PORE_DNA_R10_400 = 4
};

/* Call-level status. INVALID_ARGUMENT corresponds to std::invalid_argument (-> Python
 * ValueError), RUNTIME to std::runtime_error (-> Python RuntimeError) in the reference. */
enum dyn_status {
  DYN_OK = 0,
  DYN_ERR_INVALID_ARGUMENT = 1,
  DYN_ERR_RUNTIME = 2,
  DYN_ERR_DEVICE = 3,      /* HIP runtime failure / no GPU / kernel image missing */
  DYN_ERR_OUT_OF_MEMORY = 4
};

/* Per-read status: a failing read never aborts its batch (segment.py:160-187). */
enum dyn_read_status {
  DYN_READ_OK = 0,
  DYN_READ_SIGNAL_EMPTY = 1,     /* "Signal is empty"                        aligner.cpp:149-152 */
  DYN_READ_SEQ_SHORT = 2,        /* "Sequence shorter than model kmer size"  aligner.cpp:154-157 */
  DYN_READ_SIGNAL_SHORT = 3,     /* "Signal too short compared to sequence"  aligner.cpp:159-163 */
  DYN_READ_INVALID_NT = 4,       /* "Invalid nucleotide: X"                  aligner.cpp:180-196 */
  DYN_READ_Z_MISMATCH = 5,       /* "Alignment failed: alignment scores do not match"  NT_aligner_api.cpp:288-291 */
  DYN_READ_TRAIN_Z_MISMATCH = 6, /* "Training failed: alignment scores do not match"   NT_aligner_api.cpp:622-625.
                                  * train() here has ONE Z (the backward sweep's); what it checks instead of |Zf - Zb| is
                                  * that Z is finite and that the posterior chain delivers all its mass to the end cell
                                  * and weight 1 per sample. Same outcome for inf / NaN samples; a sample ~1e6 model
                                  * standard deviations out (|Z| ~ 1e12), where the reference's two roundings of Z
                                  * disagree and it refuses the read, trains here. DESIGN.md section 3. */
  DYN_READ_INTERNAL = 7,         /* traceback left the lattice (cannot happen once the Z check passed) */
  DYN_READ_NTK_MISMATCH = 9,     /* "NTK alignment failed: alignment scores do not match"  NTK_aligner_api.cpp:911-917:
                                    what every read that passes validation gets from a handle created with mode
                                    "resquiggle"/"ntk" -- the reference's NTKAligner fails that check on every read in this
                                    snapshot (observed with the compiled reference, tests/golden/g11_ntk_messages.json) */
  DYN_READ_TOO_LARGE = 8,        /* "Read too large for the device memory budget": this read's lattice alone exceeds
                                    the HBM budget (or 2^31 rows); the reference would raise std::bad_alloc for that
                                    read only (segment.py:172-176), so it is a per-read status, not a batch error */
  DYN_READ_BAND_TOO_WIDE = 11,   /* "Band wider than this build's 4096 band columns for a read of this length": the handle was
                                    created with band > 4 093 and the read has more than 4 093 lattice columns, so that its
                                    half band min(band / 2, columns / 2) exceeds 2 046 -- what the generic kernel's rows hold
                                    (band_reads.hip). Every other read is computed as the reference computes it: half bands up
                                    to 223 by the register sweeps, 224 .. 2 046 by the generic kernel. */
  DYN_READ_BAD_SIGNAL = 10       /* "Signal could not be decoded" (dyn_batch_align_vbz_async): a POD5 chunk of this read is
                                    corrupt, truncated or shorter than the read's [start:end) slice. In the reference the
                                    pod5 reader raises inside the worker and the listener gets ONE line for that read,
                                    "error: worker, <message>\tN: ..\tRid: ..\tSid: .." (segment.py:178-187); the CSV sink
                                    writes that form for this status. The rest of the batch is unaffected. */
};

/* or-ed into raw_dtype of the *_raw_async calls: `raw` is not one concatenated array but a table of n_reads pointers
 * (const void* const*), one per read's slice; raw_offsets still hold the prefix sums of the slice lengths. The library
 * gathers the slices into its pinned staging buffer on its helper threads -- no copy on the caller's side. */
#define DYN_RAW_SCATTERED 0x100

typedef struct dyn_aligner dyn_aligner;
typedef struct dyn_batch dyn_batch;
typedef struct dyn_multi dyn_multi;

typedef struct dyn_info {
  int32_t abi_version;
  int32_t pore;
  int32_t rna;             /* 1 for RNA pores (aligner.cpp:62-86) */
  int32_t kmer_size;
  int32_t alphabet_size;   /* inferred from the model file (aligner.cpp:118) */
  int32_t device;
  uint64_t num_kmers;      /* alphabet_size ** kmer_size */
  uint64_t half_band;      /* band / 2 (aligner.cpp:21) */
  double log_m1, log_e1, log_e2; /* NT_aligner_api.cpp:84-86 */
  uint64_t max_half_band;  /* largest half band this build computes (2 046: the generic kernel's; the tuned sweeps': 223) */
} dyn_info;

/* One output row per segment (= one CSV line of segmentation_to_string, utils.py:193-232).
 * state is always 'M' on the NT path (NT_aligner_api.cpp:424-430) and is not stored per row. */
typedef struct dyn_segment_row {
  uint32_t signal_pos;   /* Segment::signalPosition   */
  uint32_t sequence_pos; /* Segment::sequencePosition */
  double probability;    /* Segment::probability      */
} dyn_segment_row;

/* Caller-allocated result arrays for dyn_align_batch / dyn_batch_fetch.
 * Segment arrays must hold dyn_segment_capacity() entries; read i's segments start at
 * seg_offsets[i] and there are n_segments[i] of them (0 when calc_probabilities == 0 or the
 * read failed). Any pointer except Z/status may be NULL to skip that column. */
typedef struct dyn_align_out {
  double* Z;                  /* [n_reads]  Result::Z (= backward score)        */
  int32_t* status;            /* [n_reads]  dyn_read_status                      */
  char* bad_char;             /* [n_reads]  offending base for DYN_READ_INVALID_NT, else 0 */
  uint64_t* seg_offsets;      /* [n_reads+1]                                     */
  uint64_t* n_segments;       /* [n_reads]                                       */
  uint64_t* sequence_positions; /* [capacity]  aligner_bindings.cpp:59,72        */
  uint64_t* signal_positions;   /* [capacity]  aligner_bindings.cpp:60,73        */
  double* probabilities;        /* [capacity]  aligner_bindings.cpp:61,74        */
  uint8_t* states;              /* [capacity]  'M'                               */
  uint64_t capacity;
} dyn_align_out;

/* (ABI 9) Per-segment signal levels of an align(calc_probabilities = 1) job whose handle had dyn_aligner_set_event_stats
 * on when the batch was submitted: caller-allocated columns indexed like the segment arrays of dyn_align_out: read i's
 * segments at seg_offsets[i], n_segments[i] of them; rows of failed reads are 0. Over segment s's samples of the ALIGNED
 * signal x (after preprocessing, as dyn_batch_signals returns it), [signal_positions[s], signal_positions[s+1]) -- the
 * last one up to the read's end -- in the model's normalised units (not pA), L >= 1 samples:
 *   mean   = S / L, S = sum of x in chunks of 64 consecutive samples from the first (each chunk left to right from its
 *            first element, the chunk sums left to right from the first), one IEEE fp64 operation each, no FMA
 *   stdev  = sqrt(Q / L), Q = the same chunked sum of (x - mean)^2 (population standard deviation)
 *   median = s[L/2] (odd L) or (s[L/2 - 1] + s[L/2]) / 2.0 (even L) of the sorted samples, then + 0.0 */
typedef struct dyn_event_out {
  double* mean;    /* [capacity] level_mean */
  double* stdev;   /* [capacity] level_stdv */
  double* median;  /* [capacity] level_median */
  uint64_t capacity;
} dyn_event_out;

/* (added within ABI 10: a caller that must know looks the symbol up) Per-border segment quality scores of an
 * align(calc_probabilities = 1) job whose handle had dyn_aligner_set_segment_scores(a, W) with W > 0 when the batch was
 * submitted: caller-allocated columns indexed like the segment arrays of dyn_align_out; rows of failed reads are 0. For an
 * OK read, x[0 .. S) is the ALIGNED signal (what dyn_batch_signals returns; with rescaling on, the last pass's), n its output
 * rows, sp[j] row j's signal_positions, e[j] = sp[j+1] and e[n-1] = S. Units are the model's normalised units (not pA).
 *   med(v)          v non-empty, L elements sorted as s: s[L/2] (odd L) or (s[L/2 - 1] + s[L/2]) / 2.0 (even L), one IEEE
 *                   add and one IEEE divide
 *   mad(v)          med(|v_i - med(v)|), one IEEE subtraction and fabs per element
 *   median_delta[j] |med(B) - med(A)|, A = x[max(0, sp[j] - W) : sp[j]], B = x[sp[j] : min(sp[j] + W, S)]
 *   mad_delta[j]    |mad(B) - mad(A)|;  a row with sp[j] == 0 (every read's row 0) has no A: both deltas are NaN
 *   homogeneity[j]  L = e[j] - sp[j] >= 10: mad(x[sp[j] + trim : e[j] - trim]) with trim = max(L / 10, 1) in integer
 *                   division (= the reference's int(0.1 * L) for every L <= 5 000 000); otherwise NaN
 * NaN is always 0x7ff8000000000000; no result is -0.0 (fabs is last). These are the scores of the reference's
 * src/dynamont/misc/compareTools.py (processReadScores), with these deviations: the reference works on the whole raw POD5
 * signal with absolute positions and in raw units, we on the aligned slice, so windows are cut at the slice's ends; it skips
 * the first border and the last segment and casts to float32 -- given x and sp, its `scores` array equals our rows
 * 1 .. n-2 cast to float32 (tests/test_segment_scores_host.py). */
#define DYN_SEGMENT_SCORES_MAX_WINDOW 256
typedef struct dyn_score_out {
  double* median_delta;  /* [capacity] */
  double* mad_delta;     /* [capacity] */
  double* homogeneity;   /* [capacity] */
  uint64_t capacity;
} dyn_score_out;

/* (added within ABI 10: a caller that must know looks the symbol up) Per-border posterior confidence of an
 * align(calc_probabilities = 1) job whose handle had dyn_aligner_set_border_confidence(a, W) with W > 0 when the batch was
 * submitted: caller-allocated columns indexed like the segment arrays of dyn_align_out; rows of failed reads are 0. For
 * output row j of an OK read with T - 1 samples: n = j + 1 is its lattice column, r = signal_positions[j] + 1 the row of its
 * M cell, LPM(t, n) = (fM(t, n) + bM(t, n)) - Z the log-posterior of "segment n starts in row t" (NT_aligner_api.cpp:213-224),
 * -inf for every cell outside the reference's band window of row t (computeBounds, :90-108) and in row 0.
 *   border_probability[j]         exp(LPM(r, n)): the posterior mass on the called border itself
 *   border_window_probability[j]  sum over t = max(1, r - W) .. min(T - 1, r + W) of exp(LPM(t, n)): the mass within W samples
 *                                 of it; fp64, ascending t, one IEEE add per term, not clamped (may exceed 1 by rounding)
 * Over all rows t the masses of one column sum to 1. With dyn_aligner_set_rescale on, the values are the last pass's. */
#define DYN_BORDER_CONFIDENCE_MAX_WINDOW 256
typedef struct dyn_border_out {
  double* border_probability;         /* [capacity] */
  double* border_window_probability;  /* [capacity] */
  uint64_t capacity;
} dyn_border_out;

/* (added within ABI 10: a caller that must know looks the symbol up) Posterior path samples of an align(calc_probabilities = 1)
 * job whose handle had dyn_aligner_set_posterior_samples(a, K, seed) with K > 0 when the batch was submitted: K complete
 * alignments of every OK read drawn from the posterior distribution over alignments, each as its segment starts.
 * Lattice rows t = 0 .. T-1 (T - 1 samples), columns n = 0 .. N-1 (N - 1 output rows). LPM(t, n) / LPE(t, n): the log-posteriors
 * of the M and the E cell, both -inf outside the reference's band window of the row (computeBounds, NT_aligner_api.cpp:90-108),
 * LPM -inf in row 0, LPE(0, 0) = 0 -- the values dyn_border_out is defined over.
 *   u(seed, i, k, t) = (mix(mix(mix(seed + i) + k) + t) >> 11) * 2^-53, mix the SplitMix64 step
 *     z = x + 0x9E3779B97F4A7C15;  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31
 *   (all mod 2^64); i = the read's index in its batch or ticket, k = the sample, t = the row of the cell the choice is made at.
 * Sample k of read i starts in E(0, 0). While (t, n) != (T-1, N-1): a = LPM(t+1, n+1) (-inf when n+1 >= N or t+1 > T-1),
 * b = LPE(t+1, n). Both -inf: the sample is dead. Exactly one finite: that way is taken, no number is drawn. Both finite:
 * p = exp(a - LPE(t, n)) in fp64, and the walk moves iff u(seed, i, k, t) < p. A move records sample_start[k][j = n] = t -- a
 * signal position, the unit of signal_positions -- and continues in E(t+2, n+1) (an M cell has one way on); a stay continues in
 * E(t+1, n). M(t+1, n+1) has the single predecessor E(t, n), so P(move | E(t, n)) = exp(LPM(t+1, n+1) - LPE(t, n)): the samples
 * are exact draws from the posterior. A dead sample has all its entries 0xFFFFFFFF and is counted in sample_dead[i]; rows of
 * failed reads are 0.
 * Reproducibility: the same bits on every run of the same batch (same reads in the same order, same seed). The lattice's
 * log-posteriors are floats in two of its three layouts and rebuilt in fp64 in the third (the layout follows the batch's size
 * and the handle's memory budget), agreeing to 1e-6 and not to the bit: a draw within about 1e-6 p of its threshold may fall
 * differently from one layout to another. A sample depends on the read's INDEX: the same read at another place of another
 * batch gets other paths. */
#define DYN_POSTERIOR_SAMPLES_MAX 64
typedef struct dyn_sample_out {
  uint32_t* sample_start; /* [count][capacity]: sample k of output row s at k * capacity + s, rows indexed like dyn_align_out's */
  uint32_t* sample_dead;  /* [n]: dead samples of every read */
  uint64_t capacity;      /* >= dyn_segment_capacity() */
  uint64_t n;             /* >= the batch's read count */
  uint32_t count;         /* in: planes of sample_start, >= the batch's K; out: the batch's K */
} dyn_sample_out;

/* (added within ABI 10: a caller that must know looks the symbol up) Per-border credible intervals of an
 * align(calc_probabilities = 1) job whose handle had dyn_aligner_set_border_interval(a, mass) with mass > 0 when the batch was
 * submitted: how far the start of every segment could move, in samples, from the lattice's own posteriors.
 * Output row j of an ok read has lattice column n = j + 1 and called row r = signal_positions[j] + 1. LPM(t, n) is exactly the
 * value dyn_border_out is defined over: (fM(t, n) + bM(t, n)) - Z, -inf outside the reference's band window of row t
 * (computeBounds, NT_aligner_api.cpp:90-108) and in row 0. p(t) = exp(LPM(t, n)), taken as 0 where LPM is -inf, for
 * t = 1 .. T-1: the distribution of "base n starts at row t". a = (1 - mass) / 2. All sums are fp64, in ascending t, one IEEE
 * add per term, no contraction:
 *   C(t) the running sum of p;  S the sum of p over the column;
 *   A    the sum of d * p, d = t - r (exact as a double), each product one IEEE multiplication;
 *   B    the sum of (d * d) * p, d * d formed first.
 *   border_lo[j]   = (first t with C(t) >= a) - 1
 *   border_hi[j]   = (first t with C(t) >= 1 - a) - 1; if no row reaches the threshold (either one), the last in-band row of
 *                    the column, minus 1
 *   border_mean[j] = (r - 1) + A / S
 *   border_sd[j]   = sqrt(max(B / S - (A / S)^2, 0))
 * Positions are signal positions, the unit of signal_positions. The thresholds are absolute, not relative to S: S is 1 within
 * 1e-6 on the device (the lattice's log-posteriors are floats in two of its three layouts) and known only when the column
 * ends. The same bits on every run of the same batch in the same layout. Rows of failed reads are 0. */
#define DYN_BORDER_INTERVAL_MIN_MASS 0.01
#define DYN_BORDER_INTERVAL_MAX_MASS 0.999
typedef struct dyn_border_interval_out {
  uint32_t* border_lo;  /* [capacity] each, rows indexed like dyn_align_out's */
  uint32_t* border_hi;
  double* border_mean;
  double* border_sd;
  uint64_t capacity;    /* >= dyn_segment_capacity() */
} dyn_border_interval_out;

/* (added within ABI 10: a caller that must know looks the symbol up) Posterior-weighted per-base levels and expected dwell of an
 * align(calc_probabilities = 1) job whose handle had dyn_aligner_set_soft_levels(a, 1) when the batch was submitted: what level
 * the pore showed for every base and for how many samples, weighted by the lattice's own posteriors instead of cut at the called
 * borders -- the per-base terms of dyn_batch_train's per-k-mer sums, additive over reads and reference positions.
 * An ok read has signal x, T = len(x) + 1 lattice rows and N columns; sample x[t - 1] belongs to row t. Output row j is lattice
 * column n = j + 1. LPM(t, n) and LPE(t, n) are the log-posteriors of the cell's M and E state, LPM exactly the value
 * dyn_border_out is defined over and LPE its twin ((fE(t, n) + bE(t, n)) - Z); both are -inf outside the reference's band window
 * of row t (computeBounds, NT_aligner_api.cpp:90-108) and in row 0.
 *   pM = exp(LPM(t, n)), pE = exp(LPE(t, n))     (0 where the log is -inf)
 *   g(t)      = pM + pE                           the posterior that sample t - 1 belongs to base n
 *   weight[j] = sum over t = 1 .. T-1 of g(t)
 *   sum[j]    = sum of g(t) * x[t - 1]
 *   sumsq[j]  = sum of (g(t) * x[t - 1]) * x[t - 1]
 * The grouping of sumsq is the reference's own (posterior * obs * obs in runTraining). Every sum is fp64, in ascending t, g formed
 * first, one IEEE operation per step, no contraction. x is the signal the lattice was computed on: normalised, and with
 * dyn_aligner_set_rescale the last pass's. Summed over the rows of equal k-mer the three columns are the read's share of
 * dyn_train_out's weight / sum / sumsq. Derived values, as the CSV columns and the Python binding give them:
 *   soft_dwell = weight;  soft_mean = sum / weight;  soft_stdv = sqrt(max(sumsq / weight - soft_mean^2, 1e-12))
 * (the clamp is the reference's M-step clamp; with weight == 0 mean and stdv are NaN). The same bits on every run of the same
 * batch in the same layout. Rows of failed reads are 0. */
typedef struct dyn_soft_level_out {
  double* weight;     /* [capacity] each, rows indexed like dyn_align_out's */
  double* sum;
  double* sumsq;
  uint64_t capacity;  /* >= dyn_segment_capacity() */
} dyn_soft_level_out;

/* (added within ABI 10: a caller that must know looks the symbol up) Per-read site calls of an align(calc_probabilities = 1) job
 * whose handle had dyn_aligner_set_site_calls(a, 1) when the batch was submitted: every output row scored against the per-site
 * model of dyn_aligner_set_site_model. Row j of an ok read has the site id s of base j + kmer_size / 2
 * (dyn_aligner_stage_site_ids) and the event mean m -- level_mean of dyn_event_out, bit for bit. With the model row (pi1, mu0,
 * mu1, var0, var1) of s:
 *   site_z           = (m - mu0) / sqrt(var0)
 *   site_probability = p_1 / (p_0 + p_1), p_k = pi_k / sqrt(var_k) * exp(q_k - max(q_0, q_1)), q_k = -0.5 * ((m - mu_k)^2 / var_k),
 *                      pi_0 = 1 - pi1: the E-step of dyn_aligner_site_mixture at x = m, one IEEE fp64 operation per operation,
 *                      the library's strict exp (one evaluation; the other factor is exactly 1)
 * Both are the NaN 0x7FF8000000000000 ("no call") when no ids were staged, no model was uploaded, s is DYN_SITE_NONE or >=
 * num_sites, the row is one the per-site table would skip (m not finite or m * m >= 2^64), a sparse table has no bucket for s, or
 * the model row is not set (var0 > 0, mu0 and var0 finite); site_probability also when the row is not two-component (0 < pi1 < 1,
 * var1 > 0, mu1 and var1 finite). The same bits on every launch path. Rows of failed reads are 0. */
typedef struct dyn_site_call_out {
  double* site_probability; /* [capacity] each, rows indexed like dyn_align_out's */
  double* site_z;
  uint64_t capacity;        /* >= dyn_segment_capacity() */
} dyn_site_call_out;

/* (ABI 10) Per-read signal rescaling of an align(calc_probabilities = 1) job whose handle had dyn_aligner_set_rescale(a, K)
 * with K > 0 when the batch was submitted. Read r is aligned K + 1 times. x0 = its preprocessed signal (what
 * dyn_batch_signals returns with the switch off); A_0 = 0.0, B_0 = 1.0; pass k = 0 .. K aligns x_k, x_0 = x0 and
 * x_k[i] = (x0[i] - A_k) / B_k (one IEEE subtraction, one IEEE division per sample). After pass k < K, for a read whose
 * status is OK, over its n output rows in the order of dyn_align_out:
 *   y_j = the row's level_mean over x_k (dyn_event_out: chunks of 64 samples)
 *   m_j = the model level_mean of the k-mer whose emission scored the segment (the row's motif: lattice column n = j + 1,
 *         basepos = n - 1 + k/2), from the handle's table the alignment scores with (dyn_aligner_set_model included)
 *   mbar = S(m) / n, ybar = S(y) / n, Sxx = S((m - mbar)^2), Sxy = S((m - mbar) * (y - ybar)), b = Sxy / Sxx,
 *   a = ybar - b * mbar
 * S is a sum over the rows in chunks of 64 consecutive rows, each chunk left to right, the chunk sums left to right; every
 * operation one IEEE fp64 operation, no FMA. The fit is applied only if n >= 16, Sxx > 0, a and b are finite,
 * 0.5 <= b <= 2.0 and |a| <= 2.0: A_{k+1} = A_k + B_k * a (multiply, then add), B_{k+1} = B_k * b. Otherwise the read keeps
 * its transform and all its later fits are skipped too. A read that fails in a pass gets no fit; its status and message are
 * those of its last pass. Every result of the batch (rows, Z, probabilities, dyn_event_out, dyn_batch_signals) is that of
 * the last pass, over x_K. */
#define DYN_RESCALE_MAX_ITERS 8
typedef struct dyn_rescale_out {
  double* shift;           /* [n] A_K (0.0 for reads that were never fitted) */
  double* scale;           /* [n] B_K (1.0 for reads that were never fitted) */
  int32_t* iters_applied;  /* [n] fits applied */
  uint64_t n;              /* entries of each array: at least the batch's read count */
} dyn_rescale_out;

/* (added within ABI 10) Band-margin diagnostics: how close the called path of a read came to a REAL edge of its band, for
 * every ok read of an align(calc_probabilities = 1) job whose handle had dyn_aligner_set_band_margin(a, 1) when the batch was
 * submitted. Row t of the lattice is banded around mid(t) = size_t(t * N / T) (one fp64 product, truncated) with
 * bw = min(band / 2, N / 2) columns on either side. Output row j (column n = j + 1) covers the lattice rows from its
 * signal_position + 1 up to the next row's (the last one up to T = signal length + 1).
 *   lower edge: real at row t iff mid(t) - bw >= 2; slack n - (mid(t) - bw)
 *   upper edge: real at row t iff mid(t) + bw + 1 < N; slack (mid(t) + bw) - n
 *   an edge that is not real is the lattice's own border and contributes nothing
 * low / high: the minimum slack over all path rows where that edge is real, DYN_BAND_MARGIN_NONE where it never is;
 * edge_rows: the path rows with a real slack of 0 (a row where both are 0 counts once). A failed read gets NONE, NONE, 0.
 * A margin of 0 says that the band, not the signal, may have decided the alignment: align the read again at a wider band.
 * With dyn_aligner_set_rescale on, the values are the last pass's. */
#define DYN_BAND_MARGIN_NONE 0xFFFFFFFFu
typedef struct dyn_band_margin_out {
  uint32_t* low;        /* [n] band_margin_low */
  uint32_t* high;       /* [n] band_margin_high */
  uint32_t* edge_rows;  /* [n] band_edge_rows */
  uint64_t n;           /* entries of each array: at least the batch's read count */
} dyn_band_margin_out;

/* Per-read training results (replaces dynamont::TrainingResult, aligner.hpp:48-53, whose
 * pybind form is a list of num_kmers dicts per read, aligner_bindings.cpp:86-107). The emission
 * update is returned SPARSE: only k-mers with weight > 0 (all others keep the loaded model,
 * NT_aligner_api.cpp:531-534). Read i's entries start at em_offsets[i]; there are em_count[i]. */
typedef struct dyn_train_out {
  double* Z;              /* [n_reads] */
  int32_t* status;        /* [n_reads] */
  char* bad_char;         /* [n_reads] or NULL */
  double* transitions;    /* [3*n_reads] m1, e1, e2 as probabilities (NT_aligner_api.cpp:703-722) */
  uint64_t* em_offsets;   /* [n_reads+1] */
  uint64_t* em_count;     /* [n_reads] */
  int32_t* em_code;       /* [capacity] k-mer code */
  double* em_mean;        /* [capacity] */
  double* em_stdev;       /* [capacity] */
  double* em_weight;      /* [capacity] or NULL: expected count w (sufficient statistic)  */
  double* em_sum;         /* [capacity] or NULL: sum of gamma*x                            */
  double* em_sumsq;       /* [capacity] or NULL: sum of gamma*x*x                          */
  double* trans_counts;   /* [2*n_reads] or NULL: expected #(E->M) and #(E->E) transitions (linear) */
  uint64_t capacity;      /* >= dyn_segment_capacity() */
} dyn_train_out;

/* Timings of the last dyn_batch_align / dyn_batch_train on a batch, measured with HIP events on the
 * stream the kernels were launched on. All reads of a batch run in ONE launch of persistent waves
 * (k_read_queue: per read backward -> forward -> Z check -> traceback), so the per-phase figures are
 * that launch's duration split by the share of wave time each phase took (device cycle counters). */
typedef struct dyn_timing {
  double ms_total;       /* read-queue launch + per-segment kernels */
  double ms_dp;          /* the read-queue launch alone */
  double ms_backward;    /* ms_dp x share of wave time in backward sweeps */
  double ms_forward;     /* ms_dp x share in forward sweeps (forward + posterior + posterior-Viterbi | training sums) */
  double ms_trace;       /* ms_dp x share in traceback / write-back, + k_median + k_final (+ k_pool_stats) */
  double wave_wait_share;  /* share of wave time spent waiting for lattice pages or the queue lock */
  double wave_occupancy;   /* sum of wave lifetimes / (waves x longest lifetime): 1 = every wave busy to the end */
  uint64_t cells;        /* in-band lattice cells processed: sum over ok reads of T*min(2bw+1,N) */
  uint64_t samples;      /* sum of signal lengths over ok reads */
  uint64_t reads_ok;
  uint32_t launches;     /* read-queue launches (1; 0 for a batch without an ok read): strict and plain reads share one launch */
  uint32_t lp_inplace;   /* 1: the page pool could not hold a separate-layout lattice (12 B per band slot) for every
                            wave, the posteriors overwrote the backward rows in place (8 B per slot, slower sweep) */
  uint32_t pool_pages;   /* pages in the lattice pool */
  uint32_t page_rows;    /* lattice rows per page */
  uint32_t n_static;     /* reads whose pages were reserved by the host (first round) */
  uint32_t n_waves;      /* persistent waves launched */
  uint32_t reads_strict; /* reads that went through the strict kernels (dyn_aligner_set_strict) */
  uint32_t reserved;
  /* (ABI 4) the strict reads of the launch apart: their share of ms_backward / ms_forward, and how often a register of 64
   * sums had to be recomputed with the restated glibc because a certificate could not decide it */
  double ms_backward_strict;
  double ms_forward_strict;
  uint64_t cert_fallbacks;
  uint64_t cert_rows;    /* lattice rows computed in the certified arithmetic (both sweeps) */
  /* (ABI 4) Asynchronous tickets that were waiting together while the GPU was busy are MERGED into one read-queue launch
   * (a launch of fewer reads than waves cannot balance). Such a ticket reports the timing of the launch that carried it
   * (ms_*, wave_*, cert_*) and its OWN reads, cells, samples and strict reads; launch_share is its part of that launch
   * (its cells / the launch's cells; 1 for a ticket that ran alone): sum ms_dp x launch_share over tickets = GPU time,
   * sum launch_share = number of launches. */
  double launch_share;
} dyn_timing;

/* (ABI 6, additive) The RESIDENT read queue. Asynchronous align(calc_probabilities=1) tickets of at least 512 reads whose
 * lattices fit one static arena per wave do not get a kernel launch each: the handle keeps ONE launch of resident waves
 * (a "session") on a stream that owns its hardware queue, publishes ticket after ticket into it while it runs, and closes
 * it when its pipeline has run dry -- no wave idles between batches (a launch per batch, or per two or three, ends with
 * its waves up to one read apart; k_session, dynamont_amd/csrc/nt_kernels.hip). Results are those of separate launches bit
 * for bit. Such a ticket's dyn_timing reports its own wave time: ms_dp = (wave-cycles its reads took) / waves, launches =
 * 0, launch_share = 0; the sessions themselves are accounted for here -- ms is the sum of the session kernels' durations
 * (HIP events on the session stream), which is what the roofline of a run must be taken over. Everything else (training,
 * Z-only jobs, small batches with no session open, the synchronous calls) runs as one launch per batch as before; a handle
 * whose session stream cannot be created, or with DYN_NO_SESSION=1 in the environment, never opens a session.
 * Resident waves that find no work for DYN_SESSION_IDLE_S seconds (default 20) while the session is held open leave on
 * their own (`aborted`); a ticket that was published after that is published again into the next session, its results
 * unchanged (`republished`). */
typedef struct dyn_session_stats {
  uint64_t sessions;       /* closed sessions */
  uint64_t tickets, reads, cells;
  double ms;               /* sum of their kernels' durations */
  uint64_t wave_cycles_busy, wave_cycles_idle, wave_cycles_life;   /* shader-clock cycles, summed over waves and sessions */
  uint64_t waves;          /* sum over sessions of waves launched */
  uint64_t aborted;        /* sessions whose waves raised the abort word (idle watchdog) */
  uint64_t republished;    /* tickets published again because their session had aborted before it took them */
} dyn_session_stats;

/* aligner_bindings.cpp:18-32 poreTypeFromString. Unknown -> DYN_ERR_INVALID_ARGUMENT,
 * message "Unknown pore type: <s>". */
int dyn_pore_from_string(const char* s, int* pore_out, char* err, uint64_t errcap);

/* PyAligner ctor -> makeAligner -> NTAligner ctor (aligner_bindings.cpp:34-51,112-130;
 * NT_aligner_api.cpp:11-19; aligner.cpp:13-36,88-143). mode "basic" or "nt": the NT path this library accelerates.
 * mode "resquiggle" or "ntk" (-> NTKAligner, aligner_bindings.cpp:46-49) is accepted like the reference accepts it and
 * behaves like the reference's does in this snapshot: reads fail validation with the usual messages or get
 * DYN_READ_NTK_MISMATCH, training returns DYN_ERR_RUNTIME "Training is not implemented for this aligner" (aligner.cpp:
 * 38-44); no kernel runs. Any other value -> DYN_ERR_INVALID_ARGUMENT "Unknown aligner mode: <m>".
 * band: any value, as in the reference (aligner.cpp:21). The tuned sweeps hold 448 band slots per lattice row (half bands
 * up to 223: every caller in the reference fixes band = 400, segment.py:45, utils.py:161). A read whose half band
 * min(band / 2, columns / 2) exceeds that -- band > 447 AND more than 447 lattice columns -- takes a generic kernel in the
 * same batch (band_reads.hip: one workgroup per read, rows of up to 4 096 band columns in LDS, the reference's own
 * arithmetic in every cell: Z bit for bit; align, the Z-only call and train alike; a fraction of the tuned sweeps' rate).
 * Only a half band above 2 046 is refused, per read: DYN_READ_BAND_TOO_WIDE. device < 0 -> current HIP device. */
int dyn_aligner_create(const char* model_path, int pore, const char* mode, int threads,
                       uint64_t band, int device, dyn_aligner** out, char* err, uint64_t errcap);
/* The lattice pool of a destroyed handle (up to ~100 GB; allocating or freeing that much takes seconds) is PARKED per
 * device and taken over by the next handle created on that device -- the reference's training loop builds a new
 * Aligner for every batch (train.py:179,227). dyn_release_cached_memory() frees whatever is parked (all devices);
 * DYN_NO_POOL_CACHE=1 in the environment switches the parking off. */
void dyn_aligner_destroy(dyn_aligner* a);
void dyn_release_cached_memory(void);
int dyn_aligner_info(const dyn_aligner* a, dyn_info* info);
/* Totals over the handle's CLOSED sessions (dyn_session_stats above). Closes an open session first and waits until its
 * waves have left -- call it when the tickets of interest have been waited for. */
int dyn_aligner_session_stats(dyn_aligner* a, dyn_session_stats* out);
/* (ABI 7, additive) The part of dyn_session_stats.wave_cycles_idle that waves of PAGED sessions (page-starved batches: reads of
 * 100 k samples, BASELINE configs[2]) spent getting their lattice pages from the shared pool -- giving back what they held,
 * waiting for the free list to hold their request, taking it. Same units and the same closing behaviour as above. No
 * counterpart in the reference (it allocates eight T x B matrices per read, NT_aligner_api.cpp:249-262). */
int dyn_aligner_session_page_wait(dyn_aligner* a, uint64_t* wave_cycles_waiting_for_pages);
/* (ABI 8, additive) Where the resident waves' idle share sat, counted by the waves themselves (wave-cycles, summed over the
 * handle's sessions like dyn_session_stats; closes an open session first): out4[0] before a wave's first read (part of
 * wave_cycles_idle), out4[1] the part of out4[0] spent getting pages, out4[2] in a wave's LAST turn -- no read left to claim,
 * polling for the session's close; part of wave_cycles_life - busy - idle --, out4[3] the sum over the sessions of the longest
 * last turn of any wave. A finite run pays out4[2] once per session ("Paged sessions"); a stream does not.
 * No counterpart in the reference. */
int dyn_aligner_session_idle_split(dyn_aligner* a, uint64_t out4[4]);
/* enabled = 0: no resident read queue on this handle (one launch per batch, as DYN_NO_SESSION=1 does for a process).
 * enabled = 1: sessions of n_cus - reserved_cus workgroups, one per compute unit. A resident session leaves 9.5 KB of LDS and 152
 * registers per lane free on every CU it occupies: the library's own small kernels run beside it. A kernel whose workgroups need
 * more (RCCL's: 37 KB of LDS, 248-256 registers) starts beside a session iff it has NO MORE workgroups than reserved_cus
 * (reserve multiples of 8: one per XCD); one workgroup more and it waits until the session has ended (measured:
 * tools/ubench/resident_probe.hip) -- a process that runs such kernels WHILE tickets are in flight
 * reserves CUs and caps their grid (RCCL: one workgroup per channel, NCCL_MAX_NCHANNELS), accepts the wait (sessions end when
 * the handle's pipeline runs dry), or switches the queue off; bench.py --gpus N does the first and falls back to the last
 * after probing. Closes an open session first. Default: enabled, nothing reserved (DYN_SESSION_RESERVE_CUS in the
 * environment changes the default). */
int dyn_aligner_set_session_mode(dyn_aligner* a, int enabled, int reserved_cus);
/* Dense model table in k-mer-code order, (mean, stdev) interleaved, 2*num_kmers doubles. */
int dyn_aligner_model(const dyn_aligner* a, double* out2n);
/* Replace the model table (same layout as dyn_aligner_model: k-mer-code order, (mean, stdev) interleaved). The handle
 * then behaves like one created from a model file holding these values -- the reference's training loop writes such a
 * file after every batch and builds a new Aligner from it (train.py:179,221-227); a float64 survives that round trip
 * through its shortest decimal representation unchanged. Waits for the handle's device to be idle; no asynchronous
 * ticket of the handle may be pending. */
int dyn_aligner_set_model(dyn_aligner* a, const double* in2n);
/* Upper limit on HBM used for lattice workspaces (bytes; 0 = 90 % of free memory). */
int dyn_aligner_set_mem_budget(dyn_aligner* a, uint64_t bytes);
/* Strict mode (affects align with calc_probabilities only). The reference's traceback takes exact fp64 comparisons
 * (NT_aligner_api.cpp:445-448). Where two neighbouring lattice columns carry the same emission parameters (every RNA
 * read that starts with the polyA pad + A, any homopolymer of k+1 bases, distinct k-mers with coinciding table entries)
 * moving the border between their segments leaves the exact score unchanged: such a comparison is a tie in exact
 * arithmetic and the reference's choice rests on the last bits of glibc's exp/log1p inside logPlus (aligner.cpp:
 * 276-285). Entries within 1e-9 of each other in mean and in stdev are treated alike: there the comparison is no
 * exact tie, but its margin is of the order of the gap and can lie below what the plain arithmetic resolves. The plain kernels use a table softplus that is <= 1 ulp away from those and reproduce 3 397 of the 3 400
 * such reads of tests/golden/g10_ties.npz. The strict kernels reproduce the reference's sums bit for bit at 1.3-1.4x
 * the price of a row ("certified arithmetic", dynamont_amd/csrc/dp_math_strict.hpp): the emission's quotient formed
 * exactly from stdev and 1/stdev, each logPlus from the table softplus plus a certificate that its rounded sum cannot
 * depend on the last bits of the softplus, and glibc 2.35's x86-64 exp (FMA variant) / fdlibm log1p restated operation
 * by operation for the ~1e-4 of the sums the certificate cannot decide.
 *   mode 0: off
 *   mode 1: (DEFAULT) every read with such a pair of columns (dyn_tie_rows != 0) takes the strict backward sweep (Z
 *           becomes bit-identical) and the strict arithmetic for the forward rows up to the one in which the last tied
 *           pair has left the band -- the Viterbi values of a row depend on forward values of earlier rows only, so every
 *           decision up to there is the reference's own, and no decision is taken on a column outside the band
 *   mode 2: every read, every row of both sweeps
 * Returns DYN_ERR_INVALID_ARGUMENT for an unknown mode, and for modes 1/2 on a model holding a stdev whose significand
 * is all ones (no division-free exact quotient exists for that one divisor; no decimal parses to it). */
int dyn_aligner_set_strict(dyn_aligner* a, int mode);
/* train(): which reads are refused. Off (default): the posterior chain's own rule -- Z finite, all mass delivered to the
 * end cell, weight 1 per sample (see DYN_READ_TRAIN_Z_MISMATCH). On: additionally the reference's rule,
 * |Zf - Zb| / (T x B) > 1e-8 -> "Training failed: alignment scores do not match" (NT_aligner_api.cpp:619-625), with Zf
 * from one more (Z-only, no lattice traffic) forward sweep per read: `.errors` then lists the pathological reads the
 * reference lists (a sample ~1e6 model standard deviations out), at ~25 % more time per train() launch. */
int dyn_aligner_set_train_zcheck(dyn_aligner* a, int on);
/* (ABI 9) align(calc_probabilities = 1) also computes the per-segment signal levels (dyn_event_out) on the device, behind
 * the per-segment kernels, for every batch or ticket SUBMITTED while it is on (dyn_batch_align, dyn_batch_align*_async);
 * 3 x 8 bytes of device memory per segment row for those batches only. Default off: nothing else changes. */
int dyn_aligner_set_event_stats(dyn_aligner* a, int on);
/* (ABI 10) align(calc_probabilities = 1) of every batch or ticket SUBMITTED while iters > 0 runs 1 + iters passes with a
 * per-read refit of the signal's shift and scale between them (dyn_rescale_out), all on the device with no host round trip.
 * iters = 0 .. DYN_RESCALE_MAX_ITERS, default 0 = off (nothing changes); DYN_ERR_INVALID_ARGUMENT + message outside that
 * range. Z-only jobs and train() ignore it. Such tickets always take one launch per batch, never the resident session.
 * Each pass costs about one alignment; device memory: a copy of the batch's signal, 32 bytes per read, 8 per segment row.
 * dyn_multi_*: set it on each device's handle (dyn_multi_handle). */
int dyn_aligner_set_rescale(dyn_aligner* a, int iters);
/* (added within ABI 10: a caller that must know looks the symbol up) align(calc_probabilities = 1) also computes the band
 * margins (dyn_band_margin_out) on the device, behind the per-segment kernels, for every batch or ticket SUBMITTED while it is
 * on; 12 bytes of device memory per read for those batches only. Such tickets stay in the resident session and merge with
 * tickets that did not ask. Default off: nothing is allocated, launched or changed. DYN_ERR_INVALID_ARGUMENT for a handle of
 * mode "ntk" / "resquiggle", DYN_ERR_DEVICE for one without a device. dyn_multi_*: set it on each
 * device's handle (dyn_multi_handle). */
int dyn_aligner_set_band_margin(dyn_aligner* a, int on);
/* (added within ABI 10) align(calc_probabilities = 1) also computes the per-border segment scores (dyn_score_out) with a
 * window of `window` samples on the device, behind the per-segment kernels, for every batch or ticket SUBMITTED while
 * window > 0; 4 x 8 bytes of device memory per segment row for those batches only. window = 0 ..
 * DYN_SEGMENT_SCORES_MAX_WINDOW, default 0 = off: nothing is allocated, launched or changed. DYN_ERR_INVALID_ARGUMENT +
 * message outside that range. Tickets merge into one launch only with tickets of the same window. */
int dyn_aligner_set_segment_scores(dyn_aligner* a, int window);
/* (added within ABI 10) align(calc_probabilities = 1) also computes the per-border posterior confidence (dyn_border_out)
 * with a window of `window` rows, on the device behind every read's traceback while its lattice is still in place, for every
 * batch or ticket SUBMITTED while window > 0; 2 x 8 bytes of device memory per segment row for those batches only.
 * window = 0 .. DYN_BORDER_CONFIDENCE_MAX_WINDOW, default 0 = off: nothing is allocated or changed, and every launch is the
 * one it would have been. DYN_ERR_INVALID_ARGUMENT + message outside that range. A ticket submitted with window > 0 takes
 * one launch per batch (not the resident session) and merges only with tickets of the same window. */
int dyn_aligner_set_border_confidence(dyn_aligner* a, int window);
/* (added within ABI 10) align(calc_probabilities = 1) also draws `count` posterior path samples per read (dyn_sample_out) with
 * the given seed, on the device behind every read's traceback while its lattice is still in place, for every batch or ticket
 * SUBMITTED while count > 0; 4 x count bytes of device memory per segment row for those batches only. count = 0 ..
 * DYN_POSTERIOR_SAMPLES_MAX, default 0 = off: nothing is allocated or changed, and every launch is the one it would have been.
 * DYN_ERR_INVALID_ARGUMENT + message outside that range and for count > 0 on a handle of mode ntk / resquiggle. A job or ticket
 * started while count > 0 is refused (DYN_ERR_INVALID_ARGUMENT + message) together with dyn_aligner_set_rescale(iters > 0),
 * dyn_aligner_set_auto_guide(half_width > 0), dyn_aligner_set_guide_rescue(half_width > 0) or a guided batch. Combines with
 * dyn_aligner_set_border_confidence and the per-segment riders, none of whose outputs it changes. A ticket submitted with
 * count > 0 takes one launch of its own: neither the resident session nor a merged launch. */
int dyn_aligner_set_posterior_samples(dyn_aligner* a, int count, uint64_t seed);
/* (added within ABI 10) align(calc_probabilities = 1) also computes the per-border credible intervals of the given posterior
 * mass (dyn_border_interval_out) on the device behind every read's traceback, while its lattice is still in place, for every
 * batch or ticket SUBMITTED while mass > 0; 24 bytes of device memory per segment row for those batches only. mass = 0 (the
 * default) is off: nothing is allocated or changed, and every launch is the one it would have been. Valid: 0 and
 * DYN_BORDER_INTERVAL_MIN_MASS .. DYN_BORDER_INTERVAL_MAX_MASS; anything else (a NaN too): DYN_ERR_INVALID_ARGUMENT + message,
 * and the switch stays as it was. One lattice phase runs per launch for now: a job or ticket started while mass > 0 is refused
 * (DYN_ERR_INVALID_ARGUMENT + message) together with dyn_aligner_set_border_confidence(window > 0),
 * dyn_aligner_set_posterior_samples(count > 0), dyn_aligner_set_auto_guide(half_width > 0),
 * dyn_aligner_set_guide_rescue(half_width > 0) or a guided batch. With dyn_aligner_set_rescale the values are the last pass's.
 * A ticket submitted with mass > 0 takes one launch per batch (not the resident session) and merges only with tickets of the
 * same mass. Handles of mode ntk / resquiggle ignore the switch. */
int dyn_aligner_set_border_interval(dyn_aligner* a, double mass);
/* (added within ABI 10) align(calc_probabilities = 1) also computes the posterior-weighted per-base sums (dyn_soft_level_out) on
 * the device behind every read's traceback, while its lattice is still in place, for every batch or ticket SUBMITTED while
 * on != 0; 24 bytes of device memory per segment row for those batches only. Off (the default): nothing is allocated or changed,
 * and every launch is the one it would have been. One lattice phase runs per launch for now: a job or ticket started while the
 * switch is on is refused (DYN_ERR_INVALID_ARGUMENT + message) wherever dyn_aligner_set_border_interval is -- together with
 * dyn_aligner_set_border_confidence(window > 0), dyn_aligner_set_posterior_samples(count > 0),
 * dyn_aligner_set_auto_guide(half_width > 0), dyn_aligner_set_guide_rescue(half_width > 0) or a guided batch -- and together
 * with dyn_aligner_set_border_interval(mass > 0) itself. It combines with dyn_aligner_set_rescale (the values are the last
 * pass's, over the last pass's signal), the signal levels, the segment scores, the k-mer summary and the band margins, none of
 * whose outputs it changes. A ticket submitted with the switch on takes one launch per batch (not the resident session) and
 * merges only with tickets that carry it too. Handles of mode ntk / resquiggle ignore the switch. */
int dyn_aligner_set_soft_levels(dyn_aligner* a, int on);
/* (added within ABI 10: a caller that must know looks the symbol up) Per-k-mer level summary of a run. While it is on, every output row (segment) of every read with status 0 of an
 * align(calc_probabilities = 1) batch or ticket SUBMITTED on this handle is added, on the device behind the per-segment
 * kernels, to its k-mer's entry of an accumulator that lives on the handle: six u64 per k-mer code (48 bytes x num_kmers of
 * device memory, allocated and zeroed by the first call with on != 0), as EXACT INTEGERS --
 *   n_segments, n_samples         segments and samples the k-mer's emission scored (the row's `motif`)
 *   Q1 = sum q1, Q2 = sum q2      signed 128-bit two's complement, two u64 limbs each; per segment q1 = rint(S1 * 2^40) and
 *                                 q2 = rint(S2 * 2^40) with S1 / S2 the chunked fp64 sums of x and x * x over the segment's
 *                                 samples (the samples and the summation order of dyn_event_out)
 * so the result is the same bits whatever the launch path, the merging of tickets or the order of the device's atomics. A
 * segment with S2 >= 2^64 or a non-finite sum is skipped and counted. A job counts once per time it runs; a rescaling job
 * (dyn_aligner_set_rescale) counts once, with its last pass's signal. Default off: nothing is allocated, launched or changed.
 * DYN_ERR_INVALID_ARGUMENT for a handle of mode "ntk" / "resquiggle", DYN_ERR_DEVICE for one without a device. */
int dyn_aligner_set_kmer_summary(dyn_aligner* a, int on);
/* The accumulator as it stands after every job that has COMPLETED (dyn_batch_align returned, dyn_batch_wait returned); with
 * jobs still in flight it is defined only up to those jobs. Arrays of num_kmers (dyn_info); totals: reads_ok, segments,
 * samples (both of the segments added), skipped_segments. DYN_ERR_INVALID_ARGUMENT when the switch was never on. */
int dyn_aligner_kmer_summary_fetch(dyn_aligner* a, uint64_t* n_segments, uint64_t* n_samples, uint64_t* q1_lo, uint64_t* q1_hi,
                                   uint64_t* q2_lo, uint64_t* q2_hi, uint64_t totals[4]);
/* Zeroes the accumulator and the totals (same conditions as the fetch). */
int dyn_aligner_kmer_summary_reset(dyn_aligner* a);
/* (added within ABI 10: a caller that must know looks the symbol up) Per-site level summary of a run, keyed by caller-supplied
 * site ids. A SITE ID is a uint32 the caller supplies per BASE of every sequence, in aligner
 * orientation, packed exactly like `seqs` (ids[0] belongs to the character at seq_offsets[0]; one id per character, for RNA
 * the pad included); DYN_SITE_NONE = "this base has no site". Output row j of a read -- the row whose sequence_pos is
 * j + kmer_size / 2 -- belongs to site ids[j + kmer_size / 2]. While the switch is on, every output row of every read with
 * status 0 of an align(calc_probabilities = 1) batch or ticket SUBMITTED on this handle WITH STAGED IDS is added, on the device
 * behind the per-segment kernels, to its site's entry of a table that lives on the handle: seven u64 per site (56 bytes x
 * num_sites of device memory), as EXACT INTEGERS --
 *   n_rows, n_samples, dwell_sq   rows (one per read and row: the coverage), sum of their sample counts L, sum of L * L mod 2^64
 *   M1 = sum m1, M2 = sum m2      signed 128-bit two's complement, two u64 limbs each; per row m = S1 / L (dyn_event_out's
 *                                 level_mean, bit for bit), m1 = rint(m * 2^40), m2 = rint((m * m) * 2^40)
 * so the table is the same bits whatever the launch path, the merging of tickets or the order of the device's atomics. The unit
 * is the read's event mean, one observation per read and site. A row whose id is DYN_SITE_NONE is left out and counted in
 * rows_without_site; one with id >= num_sites, a non-finite m or m * m >= 2^64 is left out and counted in rows_skipped.
 * num_sites = 0 turns the switch off (the table stays and can be fetched); num_sites > 0 (below DYN_SITE_NONE) turns it on, and
 * allocates and zeroes the table when the handle has none of that size: a call with ANOTHER size first waits for every job in
 * flight on the handle, then frees the old table. The table counts against dyn_aligner_set_mem_budget (a table larger than the
 * budget: DYN_ERR_OUT_OF_MEMORY) and against what the lattice pool may take. A job counts once per time it runs; a rescaling
 * job counts once, with its last pass's signal; under the guide rescue the summary runs once, behind the rescue. A job with the
 * switch on and nothing staged adds nothing. Default off: nothing is allocated, launched or changed. DYN_ERR_INVALID_ARGUMENT
 * for a handle of mode "ntk" / "resquiggle" or num_sites >= DYN_SITE_NONE, DYN_ERR_DEVICE for a handle without a device,
 * DYN_ERR_OUT_OF_MEMORY when the table does not fit. */
#define DYN_SITE_NONE 0xFFFFFFFFu
int dyn_aligner_set_site_summary(dyn_aligner* a, uint64_t num_sites);
/* The site ids of the NEXT batch-creating call on this handle: dyn_batch_create[_raw], dyn_align_batch or
 * dyn_batch_align[_raw|_vbz]_async (dyn_train_batch and the train tickets consume and ignore them, as a Z-only job does). That
 * call consumes them whether it succeeds or not. `count` must equal that call's seq_offsets[n] - seq_offsets[0], otherwise that
 * call fails with DYN_ERR_INVALID_ARGUMENT. Nothing is copied here: the array must stay valid as long as `seqs` must (a
 * synchronous call: until it returns; a ticket: until dyn_batch_wait has returned). Staging again replaces what was staged. */
int dyn_aligner_stage_site_ids(dyn_aligner* a, const uint32_t* site_ids, uint64_t count);
/* The columns of the sites [lo, hi) of the table as it stands after every job that has COMPLETED (the conditions of
 * dyn_aligner_kmer_summary_fetch); arrays of hi - lo. totals: reads_ok (ok reads of the jobs that added), rows_added,
 * samples_added, rows_without_site, rows_skipped. DYN_ERR_INVALID_ARGUMENT when the handle has no table or hi > num_sites. */
int dyn_aligner_site_summary_fetch(dyn_aligner* a, uint64_t lo, uint64_t hi, uint64_t* n_rows, uint64_t* n_samples,
                                   uint64_t* dwell_sq, uint64_t* m1_lo, uint64_t* m1_hi, uint64_t* m2_lo, uint64_t* m2_hi,
                                   uint64_t totals[5]);
/* Zeroes the table and the totals (same conditions as the fetch), and the per-site histograms when the handle has any. */
int dyn_aligner_site_summary_reset(dyn_aligner* a);
/* (added within ABI 10: a caller that must know looks the symbol up) Per-site level and dwell HISTOGRAMS beside the table
 * (INTEGRATION.md section 3): what a median, a quantile, a Kolmogorov-Smirnov test or a mixture fit per site needs and two
 * moments cannot give. `bins` in 2 .. 254 and finite lo < hi turn them on; the handle must have a table
 * (dyn_aligner_set_site_summary(a, num_sites > 0) first). Per site H = bins + 2 + 16 uint32 counters, contiguous:
 *   [under, level bin 1 .. bins, over, dwell bin 0 .. 15]           (num_sites * H * 4 bytes of device memory)
 * Every row the table ADDS (id < num_sites, a finite m with m * m < 2^64, an ok read of a job with staged ids) counts once in a
 * level counter and once in a dwell counter, in the same pass over the signal; rows counted in rows_without_site or rows_skipped
 * touch none, so per site both groups sum to n_rows. With inv_w = (double)bins / (hi - lo), formed once on the host:
 *   level   u = (m - lo) * inv_w, one IEEE subtraction and one IEEE product of the table's m (dyn_event_out's level_mean, bit
 *           for bit); u < 0: counter 0 (under); u >= bins: counter bins + 1 (over); otherwise counter 1 + (int)u
 *   dwell   min(31 - clz(L), 15) of the row's L samples: 1, 2-3, 4-7, ... 2^15 and above
 * The counters are exact integers (32-bit device-scope atomic adds) while a site has fewer than 2^32 rows -- the defined domain --
 * and the same bits whatever the launch path, the merging of tickets or the order of the atomics. bins = 0 stops the counting and
 * keeps the counters fetchable. A call that changes (bins, lo, hi) first waits for every job in flight, then starts zeroed
 * counters. dyn_aligner_set_site_summary with ANOTHER num_sites releases the histograms and turns them off (set them again);
 * num_sites = 0 stops both from growing. The counters count against dyn_aligner_set_mem_budget as the table does.
 * DYN_ERR_INVALID_ARGUMENT for bins outside 0, 2 .. 254, bounds that are not finite with lo < hi (or whose bins / (hi - lo) is
 * not finite), or a handle without a table; DYN_ERR_OUT_OF_MEMORY when the counters do not fit. */
int dyn_aligner_set_site_histogram(dyn_aligner* a, int bins, double lo, double hi);
/* The counters of the sites [site_lo, site_hi) after every job that has COMPLETED (the conditions of
 * dyn_aligner_site_summary_fetch): level [n][bins + 2] and dwell [n][16], n = site_hi - site_lo. */
int dyn_aligner_site_histogram_fetch(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint32_t* level, uint32_t* dwell);
/* Quantiles of the level histograms of the sites [site_lo, site_hi), reduced on the device (the histograms themselves never
 * cross to the host). n_probs in 1 .. 8, every probs[q] in [0, 1]. Per site, over its B = bins + 2 level counters:
 *   n[site]   their sum
 *   rank      k = min(max((uint32)ceil(q * n), 1), n)      (q * n: one IEEE product)
 *   bin       the smallest counter index whose inclusive prefix sum is >= k (0: under, bins + 1: over)
 *   below     the prefix sum in front of that counter;  in_bin: that counter's value
 * rank, bin, below and in_bin are [n_sites][n_probs]. A site with n = 0 has bin = 0xFFFFFFFF and rank = below = in_bin = 0. The
 * k-th smallest event mean of the site lies in `bin`; interpolated inside it, it is
 * lo + ((bin - 1) + (rank - below - 0.5) / in_bin) * (hi - lo) / bins. */
int dyn_aligner_site_quantiles(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, const double* probs, int n_probs, uint32_t* n,
                               uint32_t* rank, uint32_t* bin, uint32_t* below, uint32_t* in_bin);
/* (added within ABI 10: a caller that must know looks the symbol up) TWO SAMPLES IN ONE TABLE. A
 * second sample is mapped with ids alone: sample c's site s gets the id c * N + s in a table of 2 N sites; nothing else about the
 * accumulation changes. The table and the counters are exact integers, so merging tables is addition:
 * dyn_aligner_site_summary_add adds host columns -- a table saved by another run, for instance -- into the sites [lo, hi) of the
 * device table: n_rows, n_samples and dwell_sq mod 2^64, M1 and M2 as 128-bit two's complement (the low limb's carry goes into
 * the high limb, mod 2^128), and, when `level` [n][bins + 2] and `dwell` [n][16] are given (both or neither), every counter mod
 * 2^32; `totals` (may be NULL: adds none) is added to the table's five totals. The adds are the filling kernels' own device-scope
 * atomics: a job still in flight loses no update. The conditions and error texts of dyn_aligner_site_summary_fetch /
 * dyn_aligner_site_histogram_fetch; counters given on a handle without histograms, or one given without the other:
 * DYN_ERR_INVALID_ARGUMENT. An empty window is DYN_OK and touches nothing. */
int dyn_aligner_site_summary_add(dyn_aligner* a, uint64_t lo, uint64_t hi,
    const uint64_t* n_rows, const uint64_t* n_samples, const uint64_t* dwell_sq,
    const uint64_t* m1_lo, const uint64_t* m1_hi, const uint64_t* m2_lo, const uint64_t* m2_hi,
    const uint64_t totals[5],           /* may be NULL: adds none */
    const uint32_t* level, const uint32_t* dwell);   /* both NULL: the table alone; else [n][bins+2] and [n][16] */
/* (added within ABI 10) THE TABLE BY CONTENT. dyn_aligner_site_pack returns the LIVE rows among the
 * table rows [row_lo, row_hi) -- the ids of a dense table, the buckets [0, capacity) of a sparse one -- as records, compacted on
 * the device so that only the records cross to the host:
 *   site[i]      the row's id (dense: the row; sparse: the bucket's key)
 *   cells[i][7]  n_rows, n_samples, dwell_sq, m1_lo, m1_hi, m2_lo, m2_hi
 *   level[i][bins + 2], dwell[i][16]   the row's counters, when both are given (both or neither)
 * A row is live iff its id lies in [site_lo, site_hi) and any of its 7 cell words or -- when the counters are asked for -- of its
 * bins + 2 + 16 counters is non-zero; a key alone (dyn_aligner_set_site_model inserts such keys) makes no row live. The records
 * stand in ascending row order (so ascending id for a dense table) and are the same bytes every time for a given table. *count
 * gets the number of live rows whatever cap is; cap < *count copies NOTHING and is DYN_ERR_INVALID_ARGUMENT (call again with
 * *count). The conditions of dyn_aligner_site_summary_fetch (completed jobs; dyn_aligner_site_histogram_fetch's when counters are
 * asked for) -- and the tickets in flight when the call is made are waited for first: the records are the table behind every
 * job submitted before the call. row_hi above the table's rows, or [site_lo, site_hi) no range of the table's ids:
 * DYN_ERR_INVALID_ARGUMENT. An empty range of rows or of ids is DYN_OK with *count = 0 and touches nothing, the device
 * included; row_lo > row_hi or site_lo > site_hi is refused before the device is looked at. The rows are walked 2^20 at a time.
 * dyn_aligner_site_summary_merge adds `count` such records into the table BY KEY: record i into the row of the id
 * site[i] + offset (dense: that row; sparse: found or inserted as dyn_aligner_site_summary_add does). It adds what
 * dyn_aligner_site_summary_add adds, by the same device-scope atomics; the same id may appear any number of times in one call
 * (the records of several ranks concatenated), an all-zero record adds nothing and inserts no key, `totals` (may be NULL) is added
 * once. Every site[i] + offset must be below num_sites: otherwise DYN_ERR_INVALID_ARGUMENT, with the record's index in the text,
 * before anything is added. Records whose id finds no bucket in a sparse table are dropped whole and counted in sites_dropped;
 * the call then returns DYN_ERR_OUT_OF_MEMORY with their number in the text -- the other records were added. sites_dropped counts
 * RECORDS here: an id without a bucket that three records name counts three times. count = 0 adds the totals alone (totals
 * NULL: touches nothing). The sum of tables is the same bits whatever the order of the records or of the calls. */
int dyn_aligner_site_pack(dyn_aligner* a, uint64_t row_lo, uint64_t row_hi, uint64_t site_lo, uint64_t site_hi, uint64_t cap,
    uint32_t* site, uint64_t* cells,     /* [cap], [cap][7] */
    uint32_t* level, uint32_t* dwell,    /* both NULL: the table alone; else [cap][bins+2] and [cap][16] */
    uint64_t* count);
int dyn_aligner_site_summary_merge(dyn_aligner* a, uint64_t count, const uint32_t* site, uint64_t offset, const uint64_t* cells,
    const uint64_t totals[5],           /* may be NULL: adds none */
    const uint32_t* level, const uint32_t* dwell);   /* both NULL: the table alone; else [count][bins+2] and [count][16] */
/* Compares the sites [site_lo, site_hi) with the sites starting at other_lo, pair by pair, on the device: the histograms never
 * cross to the host. Pair i: A = site_lo + i, B = other_lo + i; a[e], b[e] their Bc = bins + 2 level counters, PA[e], PB[e] the
 * inclusive prefix sums (uint32: fewer than 2^32 rows per site is the defined domain), nA = PA[Bc - 1], nB = PB[Bc - 1]. Per counter
 *   x[e] = (uint64)PA[e] * nB,  y[e] = (uint64)PB[e] * nA,  d[e] = x[e] > y[e] ? x[e] - y[e] : y[e] - x[e]
 * (the product of two uint32 cannot overflow a uint64), and per pair
 *   level_num    max_e d[e]
 *   level_at     the SMALLEST e with d[e] == level_num
 *   level_side   +1 if x[at] > y[at] (A's distribution function is ahead: A's levels are lower), -1 if x[at] < y[at], 0 when
 *                level_num == 0
 *   nA == 0 or nB == 0: level_num = 0, level_at = 0xFFFFFFFF, level_side = 0
 * and the same three over the 16 dwell counters with the dwell counters' own totals: dwell_num, dwell_at, dwell_side.
 * n_a = nA, n_b = nB. All arrays of site_hi - site_lo. The binned Kolmogorov-Smirnov statistic is D = level_num / (nA * nB); the
 * host forms it as (double)level_num / ((double)nA * (double)nB): three roundings -- level_num to double (exact below 2^53), the
 * product nA * nB (exact below 2^53), the quotient; NaN where either side is empty. D is the distance between the two
 * distribution functions evaluated AT THE BIN EDGES ONLY: it never exceeds the distance over the raw event means, and falls
 * short of it by at most max_e max(a[e] / nA, b[e] / nB) -- at a point inside bin e one distribution function has grown by at most
 * its bin share since the edge. Choose the bins accordingly. Every output is an integer; integer adds, products and maxima do
 * not depend on order, so the comparison is the same bits on every launch path. The two windows may lie anywhere in the table, in
 * either order, and may overlap. The conditions and error texts of dyn_aligner_site_quantiles; other_lo + (site_hi - site_lo) >
 * num_sites: DYN_ERR_INVALID_ARGUMENT with a text of its own. An empty window is DYN_OK and touches nothing. */
int dyn_aligner_site_compare(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint64_t other_lo,
    uint32_t* n_a, uint32_t* n_b, uint64_t* level_num, uint32_t* level_at, int32_t* level_side,
    uint64_t* dwell_num, uint32_t* dwell_at, int32_t* dwell_side);
/* Fits, per pair of the sites [site_lo, site_hi) and the sites starting at other_lo (UINT64_MAX: no second sample, all of B's
 * counters count as 0), a mixture of two Gaussians to the POOLED level counters by EM on the device, and splits each side's rows
 * between the two components: the histograms never cross to the host. Pair i: A = site_lo + i, B = other_lo + i; a[e], b[e] their
 * Bc = bins + 2 level counters (e = 0 under, e = Bc - 1 over; the dwell counters are not used). Every floating-point operation is
 * one IEEE fp64 operation in the order written; exp is the library's strict exp (every argument is <= 0).
 *   w = (hi - lo) / bins, vfloor = (w * w) / 12, tol_mu = tol * w, tol_pi = tol       (formed on the host)
 *   x[e] = lo + ((double)e - 0.5) * w                                                 (the bin centres)
 *   c[e] = (double)a[e] + (double)b[e] for 1 <= e <= bins, c[0] = c[Bc - 1] = 0       (exact; under and over take no part)
 *   n_a, n_b: the sums of the in-range counters of each side; out_a, out_b: under + over (uint32, mod 2^32)
 *   gsum(t): G = min(64, the power of two >= Bc, at least 4). Partial l = 0 .. G - 1 starts at +0.0 and adds t[r * G + l] in rising
 *            r (an index >= Bc adds 0.0); then for m = 1, 2, 4, .. < G every partial l adds partial l ^ m (all at once). The one
 *            summation order of the whole fit.
 *   start:   n = gsum(c); status 1 (no fit) if n < min_n. m = gsum(c * x) / n, v = gsum(c * ((x - m) * (x - m))) / n; status 1 if
 *            not v > vfloor. sd = sqrt(v), mu = (m - sd, m + sd), var = (v, v), pi = (0.5, 0.5).
 *   E-step:  A_k = pi_k / sqrt(var_k); per counter d_k = x - mu_k, q_k = -0.5 * ((d_k * d_k) / var_k), qm = q_1 > q_0 ? q_1 : q_0,
 *            p_k = A_k * exp(q_k - qm), s = p_0 + p_1, g_k = p_k / s. (One exponential is exactly 1: s > 0, no logarithm anywhere.)
 *   M-step, round it = 1 .. max_iters: t_k = c * g_k, N_k = gsum(t_k). N_0 < 1 or N_1 < 1: a component has collapsed, status 3, the
 *            parameters stay those before this round, iters = it - 1. Otherwise mu'_k = gsum(t_k * x) / N_k,
 *            var'_k = max(gsum(t_k * ((x - mu'_k) * (x - mu'_k))) / N_k, vfloor), pi'_k = N_k / (N_0 + N_1); they are adopted,
 *            iters = it, and the fit stops with status 0 when max_k |mu'_k - mu_k| <= tol_mu and |pi'_1 - pi_1| <= tol_pi.
 *            max_iters rounds without that: status 2.
 *   shares:  one more E-step with the FINAL parameters; r_a = gsum((double)a * g_1), r_b = gsum((double)b * g_1), under and over
 *            excluded: the expected number of each side's rows in component 1.
 *   labels:  component 1 is the one with the larger final mean: if mu_0 > mu_1 the two are exchanged in every output, the g of
 *            the shares included (equal means: nothing is exchanged).
 * Outputs, arrays of site_hi - site_lo: pi1, mu0, mu1, var0, var1, r_a, r_b; n_a, n_b, out_a, out_b, iters, status. Status 1: the
 * seven doubles are NaN and iters = 0. Defined domain: counters whose pooled in-range sum is below 2^53. 1 <= max_iters <= 1024,
 * tol finite and >= 0, min_n >= 2, else DYN_ERR_INVALID_ARGUMENT with a text of their own (suggested: 128, 1e-3, 8). The two
 * windows may lie anywhere in the table, in either order, and may overlap. The conditions and error texts of
 * dyn_aligner_site_compare. An empty window is DYN_OK and touches nothing. */
int dyn_aligner_site_mixture(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint64_t other_lo /* UINT64_MAX: one sample */,
    uint32_t max_iters, double tol, uint32_t min_n,
    double* pi1, double* mu0, double* mu1, double* var0, double* var1, double* r_a, double* r_b,
    uint32_t* n_a, uint32_t* n_b, uint32_t* out_a, uint32_t* out_b, uint32_t* iters, uint32_t* status);
/* The SPARSE mode of the per-site table: the table, and the histograms beside it, have `capacity` rows
 * and the handle keeps a hash map on the GPU from site id to row (uint32 keys[capacity], 0xFFFFFFFF = DYN_SITE_NONE = empty; the
 * bucket is the row; linear probing over at most min(capacity, 128) buckets). A row is taken by the first job row, or the first
 * dyn_aligner_site_summary_add site, that names the id; nothing is ever deleted, so an id is in the map with ALL of its rows or
 * absent with all of them dropped. num_sites stays the bound of the ids and of every window call and may be anything below
 * DYN_SITE_NONE whatever the memory; the memory is capacity * (4 + 56) bytes plus 4 * (bins + 2 + 16) per row of histograms. Every
 * call that reads or adds a window of sites keeps its meaning in id space: an absent id reads as zeros, and while nothing was
 * dropped a sparse handle returns the bits a dense one returns. A job row whose id finds no bucket is counted in rows_dropped AND
 * in the totals' rows_skipped. dyn_aligner_site_summary_add inserts the ids of the sites that have any non-zero word; when sites
 * found no bucket it returns DYN_ERR_OUT_OF_MEMORY with a text that gives their number (sites_dropped) -- the other sites were
 * added. Everything dyn_aligner_set_site_summary says applies: num_sites = 0 is the switch off, the same (num_sites, capacity)
 * again the switch on with nothing zeroed; another size, another capacity or the other mode waits for the jobs in flight, releases
 * table, map and histograms and starts anew; the memory budget text gives rows and bytes. dyn_aligner_site_summary_reset also
 * empties the map and zeroes its statistics. capacity = 0 with num_sites > 0: DYN_ERR_INVALID_ARGUMENT. A full map is not
 * resized: reset, or set a larger one. */
int dyn_aligner_set_site_summary_sparse(dyn_aligner* a, uint64_t num_sites, uint64_t capacity);
/* out: capacity, n_keys, rows_dropped, sites_dropped. The conditions of dyn_aligner_site_summary_fetch (completed jobs); on a dense
 * handle DYN_ERR_INVALID_ARGUMENT with a text that says so -- as for the two calls below. */
int dyn_aligner_site_map_stats(dyn_aligner* a, uint64_t out[4]);
/* The keys of the buckets [bucket_lo, bucket_hi) (0xFFFFFFFF: empty), for diagnostics and tests. */
int dyn_aligner_site_map_keys(dyn_aligner* a, uint64_t bucket_lo, uint64_t bucket_hi, uint32_t* keys);
/* The id windows [w << shift, (w + 1) << shift) that hold a key, ascending, found on the GPU: *count of them, the first
 * min(*count, cap) written to windows; more than cap is DYN_ERR_INVALID_ARGUMENT (call again with *count). 0 <= shift <= 31 and
 * at most 2^22 windows in the id space. A caller walks the table window by window without gathering the empty ones. */
int dyn_aligner_site_map_windows(dyn_aligner* a, int shift, uint64_t* windows, uint64_t cap, uint64_t* count);
/* (added within ABI 10) The per-site MODEL of a handle, beside its per-site table: five doubles per table row -- pi1, mu0, mu1,
 * var0, var1, the columns dyn_aligner_site_mixture returns --, 40 bytes per row (dense: per site; sparse: per bucket), allocated
 * and zeroed by the first upload, counted in the memory budget, released with the table when dyn_aligner_set_site_summary[_sparse]
 * names another size. A row is SET when var0 > 0 and mu0, var0 are finite (all zeros: not set).
 * dyn_aligner_set_site_model uploads the rows of the sites [site_lo, site_lo + count), staged 2^20 rows at a time, after the jobs
 * that have been enqueued (the quiescence of dyn_aligner_site_summary_add). Dense: a copy. Sparse: a set row finds or inserts the
 * bucket of its id, a row that is not set inserts no key (and clears the row of an id that has one); *dropped (may be NULL) gets the
 * number of set rows whose id found no bucket in its probe window -- they are not stored, the call is still DYN_OK.
 * DYN_ERR_INVALID_ARGUMENT with a text: no table on this handle, or the window does not lie below num_sites. count = 0 touches
 * nothing. dyn_aligner_site_model_reset zeroes the model (a handle that never uploaded one: DYN_OK). dyn_aligner_site_model_fetch
 * reads the rows of [lo, hi) back (a handle without a model, or an id without a bucket: zeros). */
int dyn_aligner_set_site_model(dyn_aligner* a, uint64_t site_lo, uint64_t count, const double* pi1, const double* mu0,
                               const double* mu1, const double* var0, const double* var1, uint64_t* dropped);
int dyn_aligner_site_model_reset(dyn_aligner* a);
int dyn_aligner_site_model_fetch(dyn_aligner* a, uint64_t lo, uint64_t hi, double* pi1, double* mu0, double* mu1, double* var0,
                                 double* var1);
/* (added within ABI 10) align(calc_probabilities = 1) jobs submitted while on also score every output row against the per-site
 * model (dyn_site_call_out, dyn_batch_fetch_site_calls). The model and the map are taken as they stand at the job's submission.
 * A job submitted while on is refused with DYN_ERR_INVALID_ARGUMENT and a text when dyn_aligner_set_site_summary[_sparse] is not
 * on, and when it is not an align(calc_probabilities = 1) job; a job that staged no ids gets NaN columns. */
int dyn_aligner_set_site_calls(dyn_aligner* a, int on);
/* The rule of mode 1 for one read, given its k-mer codes (dyn_validate_batch) and signal length: 0 = no structural tie;
 * otherwise the number of forward rows that run in the strict arithmetic (UINT32_MAX: all of them). Host only. */
uint32_t dyn_tie_rows(const dyn_aligner* a, const int32_t* kmers, uint64_t n_kmers, uint64_t signal_len);
/* Message of the last failing call on this handle (thread-unsafe like the handle itself). */
const char* dyn_aligner_last_error(const dyn_aligner* a);
/* Reference exception text for a per-read status (bad_char fills "Invalid nucleotide: X"). */
int dyn_read_strerror(int read_status, char bad_char, char* buf, uint64_t cap);

/* Number of segment rows to allocate: sum over reads of max(0, len(seq_i) - k + 1). */
uint64_t dyn_segment_capacity(const dyn_aligner* a, uint64_t n_reads, const uint64_t* seq_offsets);

/* Host front half of align()/train() only: validateInput (aligner.cpp:145-164) then
 * sequenceToKmers (aligner.cpp:166-205) per read. status/bad_char: [n_reads]. kmers_out
 * (optional): k-mer codes of read i at kmers_out[seg_offset_i ...] in the dyn_segment_capacity()
 * layout (prefix sums of max(0, len_i - k + 1)). Needs no GPU. */
int dyn_validate_batch(const dyn_aligner* a, uint64_t n_reads, const uint64_t* sig_offsets,
                       const char* seqs, const uint64_t* seq_offsets, int32_t* status,
                       char* bad_char, int32_t* kmers_out, uint64_t kmers_cap);

/* NTAligner::align for a batch of reads held in HOST memory (NT_aligner_api.cpp:230-312):
 * signals = concatenated fp64 samples, read i = [sig_offsets[i], sig_offsets[i+1]);
 * seqs = concatenated bases (aligner orientation), read i = [seq_offsets[i], seq_offsets[i+1]).
 * Equivalent to create + align + fetch + destroy of a dyn_batch. */
int dyn_align_batch(dyn_aligner* a, uint64_t n_reads, const double* signals,
                    const uint64_t* sig_offsets, const char* seqs, const uint64_t* seq_offsets,
                    int calc_probabilities, dyn_align_out* out);

/* NTAligner::train for a batch (NT_aligner_api.cpp:567-639, 462-561, 641-725).
 * pooled3n (optional, 3*num_kmers doubles, caller-zeroed or accumulated across calls) receives
 * the batch-pooled sufficient statistics sum_i (w, s1, s2) in k-mer-code order -- the quantity
 * a multi-GPU job all-reduces (BASELINE.json config 5). */
int dyn_train_batch(dyn_aligner* a, uint64_t n_reads, const double* signals,
                    const uint64_t* sig_offsets, const char* seqs, const uint64_t* seq_offsets,
                    dyn_train_out* out, double* pooled3n);

/* segmentation_to_string (src/dynamont/segmentation/utils.py:193-232) for a whole batch, multi-
 * threaded on the host. `res` is a filled dyn_align_out; seqs/seq_offsets are the aligner-orientation
 * sequences the batch was aligned with; sig_offsets[i] = sigOffset, last_index[i] = lastIndex of the
 * reference call. Read i's rows are written to out[row_begin[i] .. row_end[i]) (each read formats
 * into its own worst-case slot, so the byte ranges are not contiguous; failed reads get an empty
 * range and the caller writes their .errors line). out_cap must be >= dyn_format_csv_bound().
 * Bytes are identical to the reference's Python formatting, including f"{p:.6f}". */
uint64_t dyn_format_csv_bound(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res,
                              const char* const* readids, const char* const* signalids);
int dyn_format_csv(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res,
                   const char* seqs, const uint64_t* seq_offsets, const char* const* readids,
                   const char* const* signalids, const int64_t* sig_offsets,
                   const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                   uint64_t* row_begin, uint64_t* row_end);

/* (ABI 9) The same with the signal levels of dyn_batch_fetch_events (ev indexed like res' segment arrays): every row gets
 * ",{mean:.6f},{stdev:.6f},{median:.6f}" after "NA", the bytes of Python's f"{x:.6f}" for any finite value (negatives and
 * -0.000000 included). ev == NULL: the bytes of dyn_format_csv / dyn_format_csv_bound, which are these with ev = NULL. */
uint64_t dyn_format_csv_bound_events(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                     const char* const* readids, const char* const* signalids);
int dyn_format_csv_events(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                          const char* seqs, const uint64_t* seq_offsets, const char* const* readids,
                          const char* const* signalids, const int64_t* sig_offsets,
                          const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                          uint64_t* row_begin, uint64_t* row_end);

/* (added within ABI 10) The same with the segment scores of dyn_batch_fetch_scores as well: after the level columns (if ev
 * is given) every row gets ",{median_delta:.6f},{mad_delta:.6f},{homogeneity:.6f}", NaN as "nan" like Python's f"{x:.6f}".
 * ev and sc may each be NULL; sc == NULL: dyn_format_csv_events / dyn_format_csv_bound_events, byte for byte. */
uint64_t dyn_format_csv_bound_scores(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                     const dyn_score_out* sc, const char* const* readids, const char* const* signalids);
int dyn_format_csv_scores(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                          const dyn_score_out* sc, const char* seqs, const uint64_t* seq_offsets, const char* const* readids,
                          const char* const* signalids, const int64_t* sig_offsets,
                          const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                          uint64_t* row_begin, uint64_t* row_end);

/* (added within ABI 10) The same with the border confidence of dyn_batch_fetch_borders as well: after the score columns (if
 * sc is given) every row gets ",{border_probability:.6f},{border_window_probability:.6f}". ev, sc and bd may each be NULL;
 * bd == NULL: dyn_format_csv_scores / dyn_format_csv_bound_scores, byte for byte. */
uint64_t dyn_format_csv_bound_borders(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                      const dyn_score_out* sc, const dyn_border_out* bd, const char* const* readids,
                                      const char* const* signalids);
int dyn_format_csv_borders(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                           const dyn_score_out* sc, const dyn_border_out* bd, const char* seqs, const uint64_t* seq_offsets,
                           const char* const* readids, const char* const* signalids, const int64_t* sig_offsets,
                           const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                           uint64_t* row_begin, uint64_t* row_end);

/* (added within ABI 10) The same with the posterior samples of dyn_batch_fetch_samples as well: after the border columns (if
 * bd is given) every row gets one field ",{s_0};{s_1};...;{s_K-1}", sm->count integers: sample k's start of that segment in the
 * unit of the `start` column (the fetched value + sig_offsets[i]; 4294967295 for a dead sample). ev, sc, bd and
 * sm may each be NULL; sm == NULL: dyn_format_csv_borders / dyn_format_csv_bound_borders, byte for byte. */
uint64_t dyn_format_csv_bound_samples(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                      const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                                      const char* const* readids, const char* const* signalids);
int dyn_format_csv_samples(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                           const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm, const char* seqs,
                           const uint64_t* seq_offsets, const char* const* readids, const char* const* signalids,
                           const int64_t* sig_offsets, const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                           uint64_t* row_begin, uint64_t* row_end);

/* (added within ABI 10) The same with the credible intervals of dyn_batch_fetch_intervals as well: after every other optional
 * column each row gets ",{lo},{hi},{mean:.6f},{sd:.6f}": border_lo and border_hi as integers and border_mean in the unit of the
 * `start` column (the fetched value + sig_offsets[i]), border_sd as it is; the floats as Python's f"{x:.6f}". ev, sc, bd, sm and
 * bi may each be NULL; bi == NULL: dyn_format_csv_samples / dyn_format_csv_bound_samples, byte for byte. */
uint64_t dyn_format_csv_bound_intervals(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                        const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                                        const dyn_border_interval_out* bi, const char* const* readids,
                                        const char* const* signalids);
int dyn_format_csv_intervals(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                             const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                             const dyn_border_interval_out* bi, const char* seqs, const uint64_t* seq_offsets,
                             const char* const* readids, const char* const* signalids, const int64_t* sig_offsets,
                             const int64_t* last_index, int threads, char* out, uint64_t out_cap, uint64_t* row_begin,
                             uint64_t* row_end);

/* (added within ABI 10) The same with the soft levels of dyn_batch_fetch_soft_levels as well: after every other optional column
 * each row gets ",{soft_dwell:.6f},{soft_mean:.6f},{soft_stdv:.6f}", derived from the three sums as dyn_soft_level_out says, the
 * floats as Python's f"{x:.6f}" (a NaN as "nan"). ev, sc, bd, sm, bi and sl may each be NULL; sl == NULL:
 * dyn_format_csv_intervals / dyn_format_csv_bound_intervals, byte for byte. */
uint64_t dyn_format_csv_bound_soft(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                   const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                                   const dyn_border_interval_out* bi, const dyn_soft_level_out* sl, const char* const* readids,
                                   const char* const* signalids);
int dyn_format_csv_soft(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                        const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                        const dyn_border_interval_out* bi, const dyn_soft_level_out* sl, const char* seqs,
                        const uint64_t* seq_offsets, const char* const* readids, const char* const* signalids,
                        const int64_t* sig_offsets, const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                        uint64_t* row_begin, uint64_t* row_end);

/* (added within ABI 10) The same with the site calls of dyn_batch_fetch_site_calls as well: after every other optional column each
 * row gets ",{site_probability:.6f},{site_z:.6f}", the floats as the level columns print theirs (a NaN as "nan", an infinity as "inf" / "-inf"). Every out-struct
 * may be NULL; ca == NULL: dyn_format_csv_soft / dyn_format_csv_bound_soft, byte for byte. */
uint64_t dyn_format_csv_bound_calls(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                                    const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                                    const dyn_border_interval_out* bi, const dyn_soft_level_out* sl, const dyn_site_call_out* ca,
                                    const char* const* readids, const char* const* signalids);
int dyn_format_csv_calls(const dyn_aligner* a, uint64_t n_reads, const dyn_align_out* res, const dyn_event_out* ev,
                         const dyn_score_out* sc, const dyn_border_out* bd, const dyn_sample_out* sm,
                         const dyn_border_interval_out* bi, const dyn_soft_level_out* sl, const dyn_site_call_out* ca, const char* seqs,
                         const uint64_t* seq_offsets, const char* const* readids, const char* const* signalids,
                         const int64_t* sig_offsets, const int64_t* last_index, int threads, char* out, uint64_t out_cap,
                         uint64_t* row_begin, uint64_t* row_end);

/* Closes the gaps between the per-read ranges dyn_format_csv produced: all rows become one contiguous run at the
 * front of `out`, in read order; row_begin/row_end are updated. Returns the total byte count. */
uint64_t dyn_csv_compact(char* out, uint64_t n_reads, uint64_t* row_begin, uint64_t* row_end);

/* The text of a k-mer model file as write_kmer_model produces it (src/dynamont/segmentation/utils.py:136-152: header
 * "kmer\tlevel_mean\tlevel_stdv", then f"{kmer}\t{mean}\t{stdev}\n" per row; dynamont-train writes one per batch,
 * train.py:221-224): kmers = n rows of k characters, file order; a float64 prints as Python's repr(). Returns the
 * byte count; with out == NULL or cap too small nothing is written and the size to provide is returned. */
uint64_t dyn_format_model(const char* kmers, int k, const double* mean, const double* stdev, uint64_t n,
                          char* out, uint64_t cap);

/* ---- the output half of dynamont-resquiggle (src/dynamont/segmentation/segment.py:69-107, the listener) ----
 *
 * A sink owns `<out>.csv.zst` (ONE zstd frame at `level`, like the reference's stream writer; header line written at
 * open) and appends to `<out>.errors`. dyn_csv_sink_submit hands it a ticket of dyn_batch_align[_raw]_async and
 * returns at once: a sink thread waits for the batch, formats its rows (dyn_format_csv, bytes ==
 * utils.segmentation_to_string), compresses them on `threads` threads and writes them in submission order; reads
 * whose status is not DYN_READ_OK get the reference's line
 * "error: native, <message>\tT: <samples>\tN: <bases>\tRid: <readid>\tSid: <signalid>" (segment.py:172-176).
 * sig_offsets[i] = sigOffset of segmentation_to_string (the read's first sample in the raw signal), signal_lengths[i]
 * = its samples (lastIndex = sum). Everything passed to submit (and the ticket) must stay valid until
 * dyn_csv_sink_completed() has counted the batch; the sink never destroys a ticket. */
typedef struct dyn_csv_sink dyn_csv_sink;
int dyn_csv_sink_open(const char* csv_zst_path, const char* errors_path, int level, int threads, dyn_csv_sink** out,
                      char* err, uint64_t errcap);
/* The same sink writing a PART of a frame that several processes write (one process per GPU: every rank compresses its
 * own rows, the root only concatenates bytes -- compressing is the largest host cost of the output by far). A part with
 * `first` carries the CSV header line and the zstd frame header, a part with `last` the frame's closing block;
 * first = last = 1 is dyn_csv_sink_open. Parts are sequences of complete zstd blocks: [first part][any other parts, in any
 * order][DYN_ZSTD_FRAME_END] is ONE valid frame. */
int dyn_csv_sink_open_part(const char* csv_zst_path, const char* errors_path, int level, int threads, int first, int last,
                           dyn_csv_sink** out, char* err, uint64_t errcap);
/* (ABI 9) dyn_csv_sink_open_part with flags. DYN_CSV_EVENT_STATS: the header gains ",level_mean,level_stdv,level_median",
 * every row the three columns (dyn_format_csv_events); the sink fetches each ticket's levels after its wait, and a submit
 * whose ticket was submitted without dyn_aligner_set_event_stats on fails with DYN_ERR_INVALID_ARGUMENT. `.errors` lines
 * are unchanged. flags = 0 is dyn_csv_sink_open_part. */
#define DYN_CSV_EVENT_STATS 0x1u
/* (added within ABI 10) DYN_CSV_SEGMENT_SCORES: the header gains ",median_delta,mad_delta,homogeneity" (after the level
 * columns, if any), every row the three columns (dyn_format_csv_scores); the sink fetches each ticket's scores after its
 * wait, and a submit whose ticket was submitted with dyn_aligner_set_segment_scores off fails with
 * DYN_ERR_INVALID_ARGUMENT. */
#define DYN_CSV_SEGMENT_SCORES 0x2u
/* (added within ABI 10) DYN_CSV_BORDER_CONFIDENCE: the header gains ",border_probability,border_window_probability" (after
 * the level and score columns, if any), every row the two columns (dyn_format_csv_borders); the sink fetches each ticket's
 * columns after its wait, and a submit whose ticket was submitted with dyn_aligner_set_border_confidence off fails with
 * DYN_ERR_INVALID_ARGUMENT. (0x8, not 0x4: bit 2 stays unassigned, and a sink opened with it is
 * refused as before.) */
#define DYN_CSV_BORDER_CONFIDENCE 0x8u
/* (added within ABI 10) DYN_CSV_POSTERIOR_SAMPLES: the header gains ",sample_starts" (after the level, score and border columns,
 * if any), every row one field: the K sampled starts of its segment, integers joined by ';' (4294967295 for a dead sample); the
 * sink fetches each ticket's samples after its wait, and a submit whose ticket was submitted with
 * dyn_aligner_set_posterior_samples off fails with DYN_ERR_INVALID_ARGUMENT. Bit 0x4 and every bit above 0x10 stay refused. */
#define DYN_CSV_POSTERIOR_SAMPLES 0x10u
/* (added within ABI 10) DYN_CSV_BORDER_INTERVAL: the header gains ",border_lo,border_hi,border_mean,border_sd" after every other
 * optional column, every row the four fields of dyn_format_csv_intervals; the sink fetches each ticket's intervals after its
 * wait, and a submit whose ticket was submitted with dyn_aligner_set_border_interval off fails with DYN_ERR_INVALID_ARGUMENT.
 * (0x40, not 0x20: bits 0x4 and 0x20 stay unassigned, and a sink opened with either is refused as before; so is every bit
 * above 0x40.) */
#define DYN_CSV_BORDER_INTERVAL 0x40u
/* (added within ABI 10) DYN_CSV_SOFT_LEVELS: the header gains ",soft_dwell,soft_mean,soft_stdv" after every other optional
 * column, every row the three fields of dyn_format_csv_soft; the sink fetches each ticket's sums after its wait, and a submit
 * whose ticket was submitted with dyn_aligner_set_soft_levels off fails with DYN_ERR_INVALID_ARGUMENT. (0x200: bits 0x4, 0x20,
 * 0x80 and 0x100 stay unassigned, and a sink opened with any of them is refused as before; so is every bit above 0x200.) */
#define DYN_CSV_SOFT_LEVELS 0x200u
/* (added within ABI 10) DYN_CSV_SITE_CALLS: the header gains ",site_probability,site_z" after every other optional column, every
 * row the two fields of dyn_format_csv_calls; the sink fetches each ticket's calls after its wait, and a submit whose ticket was
 * submitted with dyn_aligner_set_site_calls off fails with DYN_ERR_INVALID_ARGUMENT. (0x800: bits 0x4, 0x20, 0x80, 0x100 and 0x400
 * stay unassigned, and a sink opened with any of them is refused as before; so is every bit above 0x800.) */
#define DYN_CSV_SITE_CALLS 0x800u
int dyn_csv_sink_open_ex(const char* csv_zst_path, const char* errors_path, int level, int threads, int first, int last,
                         uint32_t flags, dyn_csv_sink** out, char* err, uint64_t errcap);
#define DYN_ZSTD_FRAME_END "\x01\x00\x00" /* an empty last block (raw, size 0): 3 bytes; the frames carry no checksum */
int dyn_csv_sink_submit(dyn_csv_sink* s, dyn_aligner* a, dyn_batch* ticket, const dyn_align_out* res, uint64_t n_reads,
                        const char* seqs, const uint64_t* seq_offsets, const char* const* readids,
                        const char* const* signalids, const int64_t* sig_offsets, const uint64_t* signal_lengths);
/* The same with stored_bases[i] = the bases of read i's basecall AS STORED (before the RNA reversal and polyA pad), or
 * NULL: the N of a read that fails like the reference's WORKER does -- its signal cannot be read, DYN_READ_BAD_SIGNAL,
 * "error: worker, <message>\tN: <len(read)>\tRid: ...\tSid: ..." (segment.py:178-187) -- where the aligner's own failures
 * report the read in aligner orientation, pad included (segment.py:172-176). Additive: dyn_csv_sink_submit = NULL. */
int dyn_csv_sink_submit_bases(dyn_csv_sink* s, dyn_aligner* a, dyn_batch* ticket, const dyn_align_out* res, uint64_t n_reads,
                              const char* seqs, const uint64_t* seq_offsets, const char* const* readids,
                              const char* const* signalids, const int64_t* sig_offsets, const uint64_t* signal_lengths,
                              const uint32_t* stored_bases);
/* one line for `.errors` from the caller (reads that failed before they reached the aligner, segment.py:178-187) */
int dyn_csv_sink_error_line(dyn_csv_sink* s, const char* line);
/* 1 once the sink has failed (a batch error, the compressor, the output file): later submits return DYN_ERR_RUNTIME, and
 * dyn_csv_sink_close reports the first message. Lets a producer stop instead of aligning the rest of its input. */
int dyn_csv_sink_failed(dyn_csv_sink* s);
/* batches fully consumed so far */
uint64_t dyn_csv_sink_completed(const dyn_csv_sink* s);
/* blocks until `count` batches have been consumed, the sink has failed, or timeout_ms have passed (< 0: no timeout);
 * returns the batches consumed so far. What a producer that keeps a bounded number of batches in flight waits on. */
uint64_t dyn_csv_sink_wait(dyn_csv_sink* s, uint64_t count, int timeout_ms);
/* drains, closes the frame and the file, frees the sink; DYN_ERR_RUNTIME + message if any batch, compression or write
 * failed */
int dyn_csv_sink_close(dyn_csv_sink* s, uint64_t* csv_bytes, uint64_t* compressed_bytes, uint64_t* error_lines, char* err,
                       uint64_t errcap);

/* ---- the input half of dynamont-resquiggle: the basecalls, in batches (src/dynamont/segmentation/segment.py:189-258
 * generate_jobs over pysam's fetch(until_eof=True); segment.py:141-158 for the RNA orientation) ----
 *
 * A reader walks an (unaligned) BAM file -- BGZF blocks inflated a window ahead on `threads` threads, CRC-checked --
 * and dyn_bam_next returns COLUMNS for the next (up to) max_reads jobs, in file order:
 *   names / signal_ids     NUL-terminated strings back to back; *_off[i] = start of entry i, *_off[n] = total bytes
 *                          (signal id = the `pi` tag when present, else the read name)
 *   signal_uuid[16 i ..]   the signal id as the 16 bytes of its UUID (what a POD5 reads table is keyed by),
 *                          signal_uuid_ok[i] = 0 when the text is not 32 hex digits (hyphens ignored)
 *   seqs / seq_off         the basecalled sequences back to back, no separators, ready for dyn_batch_align_*:
 *                          as stored, or with DYN_JOBS_RNA reversed and with `rna_pad` in front unless the reversed read
 *                          starts with it
 *   shift, scale           the `sm`, `sd` tags (a BAM `f` value widened to double, as pysam hands it out)
 *   start, end             `sp + ts`, `sp + ns` (`sp` = 0 when absent): the slice of the raw signal
 *   file_id / files        index into the batch's distinct raw-file names (`fn`, else `f5`)
 *   bases                  bases of the record as stored (the N of the reference's error lines)
 * The arrays belong to the reader and stay valid until its next call. Reads with `qs` < min_qual (min_qual != 0) are
 * counted in dyn_bam_skipped and left out; of the reads that remain, those with index % world == rank are returned
 * (every rank of a multi-GPU run walks the file and keeps its share). n = 0: end of file. A tag generate_jobs reads
 * without asking (qs, ns, ts, fn|f5, sm, sd) and that is absent fails the call with DYN_ERR_INVALID_ARGUMENT "tag 'xx'
 * not present" (pysam: KeyError, same text); a damaged file with DYN_ERR_RUNTIME. */
typedef struct dyn_bam_reader dyn_bam_reader;
typedef struct dyn_job_batch {
  uint64_t n;
  const char* names;
  const uint64_t* name_off;
  uint64_t names_bytes;
  const char* signal_ids;
  const uint64_t* signal_id_off;
  uint64_t signal_ids_bytes;
  const uint8_t* signal_uuid;
  const uint8_t* signal_uuid_ok;
  const char* seqs;
  const uint64_t* seq_off;
  uint64_t seqs_bytes;
  const double* shift;
  const double* scale;
  const int64_t* start;
  const int64_t* end;
  uint64_t n_files;
  const char* files;
  const uint64_t* file_off;
  uint64_t files_bytes;
  const uint32_t* file_id;
  const uint32_t* bases;
} dyn_job_batch;
#define DYN_JOBS_RNA 1u
int dyn_bam_open(const char* path, int threads, const char* rna_pad, dyn_bam_reader** out, char* err, uint64_t errcap);
int dyn_bam_next(dyn_bam_reader* r, uint64_t max_reads, uint32_t flags, double min_qual, uint32_t rank, uint32_t world,
                 dyn_job_batch* out, char* err, uint64_t errcap);
uint64_t dyn_bam_skipped(const dyn_bam_reader* r);
/* (added within ABI 10: a caller that must know looks the symbol up) The mapping of a MAPPED BAM, for callers that key their
 * results by reference position (dyn_aligner_stage_site_ids; dynamont_amd/sites.py). dyn_bam_references: the header's reference
 * sequences -- n_ref of them (0: an unaligned BAM), their names NUL-terminated back to back with name_off[i] = start of name i
 * (n_ref + 1 entries), their lengths. dyn_bam_alignment: per read of the batch dyn_bam_next returned LAST, in that batch's
 * order -- the record's flag, ref_id and 0-based pos (-1: unmapped), and its CIGAR as BAM stores it (words of len << 4 | op, op
 * 0 .. 8 = MIDNSHP=X) back to back with cigar_off[i] = first word of read i (n + 1 entries). The CIGAR is as the RECORD holds
 * it, in stored orientation (a record that carries its real CIGAR in a CG tag shows the kSmN placeholder here). dyn_job_batch
 * itself does not change. The arrays belong to the reader and stay valid until its next dyn_bam_next. */
typedef struct dyn_job_alignment {
  uint64_t n;
  const uint32_t* flag;
  const int32_t* ref_id;
  const int32_t* pos;
  const uint32_t* cigar;
  const uint64_t* cigar_off;
} dyn_job_alignment;
int dyn_bam_references(dyn_bam_reader* r, uint64_t* n_ref, const char** names, const uint64_t** name_off, const uint32_t** lengths);
int dyn_bam_alignment(dyn_bam_reader* r, dyn_job_alignment* out);
void dyn_bam_close(dyn_bam_reader* r);

/* ---- staged form: inputs resident in HBM before the timed region (bench.py, pipelining) ---- */

/* Validate (aligner.cpp:145-164), k-mer-code (aligner.cpp:166-205), and upload one batch. On a DYN_DEVICE_HOST_ONLY handle:
 * validate and k-mer-code only (`signals` is not read); the batch serves dyn_batch_set_guide's validation and
 * dyn_batch_destroy, every job on it returns DYN_ERR_DEVICE. */
int dyn_batch_create(dyn_aligner* a, uint64_t n_reads, const double* signals,
                     const uint64_t* sig_offsets, const char* seqs, const uint64_t* seq_offsets,
                     dyn_batch** out);
/* The same with P1/P2 done on the device (src/dynamont/segmentation/segment.py:146-153,
 * train.py:163-170, utils.py:16-43): raw = the concatenated raw[start:end) slices of every read
 * (raw_dtype 0 = float32 picoampere `signal_pa`, 1 = int16 ADC `signal`, 2 = float64), read i =
 * [raw_offsets[i], raw_offsets[i+1]); per read x = REAL(raw); x -= shift[i]; x /= scale[i]; then the
 * Hampel filter (window, n_sigmas) -- (3, 3.0) for dynamont-resquiggle, (7, 5.0) for dynamont-train.
 * compute_f32 = 1 performs the arithmetic in float32, as NumPy does in train.py where the signal stays
 * float32; 0 = float64 as in segment.py. Results are bit-identical to the NumPy code. */
int dyn_batch_create_raw(dyn_aligner* a, uint64_t n_reads, const void* raw, int raw_dtype,
                         const uint64_t* raw_offsets, const double* shift, const double* scale,
                         int hampel_window, double hampel_n_sigmas, int compute_f32, const char* seqs,
                         const uint64_t* seq_offsets, dyn_batch** out);
/* Device-resident preprocessed signals of a batch copied back to the host (count doubles). */
int dyn_batch_signals(dyn_batch* b, double* out, uint64_t count);
void dyn_batch_destroy(dyn_batch* b);
/* Run the kernels (stream-ordered, returns after the stream is idle). Batches made by dyn_batch_create[_raw] only: a
 * ticket of the asynchronous API is a one-shot submission (it may have shared its launch, and with it every device
 * buffer, with other tickets) and gets DYN_ERR_INVALID_ARGUMENT here. dyn_batch_fetch, dyn_batch_signals,
 * dyn_batch_device_results and dyn_batch_timing serve a completed ticket whether or not its launch was shared. */
int dyn_batch_align(dyn_batch* b, int calc_probabilities);
int dyn_batch_train(dyn_batch* b);
/* Copy results of the last dyn_batch_align to the host. */
int dyn_batch_fetch(dyn_batch* b, dyn_align_out* out);
int dyn_batch_fetch_train(dyn_batch* b, dyn_train_out* out, double* pooled3n);
/* (ABI 9) Copy the signal levels of the last dyn_batch_align (or of a completed ticket, merged launch or not) into `out`
 * (capacity >= dyn_segment_capacity()). DYN_ERR_INVALID_ARGUMENT + message for a batch submitted without
 * dyn_aligner_set_event_stats on, or aligned with calc_probabilities = 0. */
int dyn_batch_fetch_events(dyn_batch* b, dyn_event_out* out);
/* (added within ABI 10) The segment scores of the batch's last align(calc_probabilities = 1) job, copied on the handle's
 * own non-blocking stream. DYN_ERR_INVALID_ARGUMENT (with a message) when the batch was submitted with
 * dyn_aligner_set_segment_scores off, or aligned with calc_probabilities = 0, or out->capacity is too small. */
int dyn_batch_fetch_scores(dyn_batch* b, dyn_score_out* out);
/* (added within ABI 10) The border confidence of the batch's last align(calc_probabilities = 1) job, copied on the handle's
 * own non-blocking stream. DYN_ERR_INVALID_ARGUMENT (with a message) when the batch was submitted with
 * dyn_aligner_set_border_confidence off, or aligned with calc_probabilities = 0, or out->capacity is too small. */
int dyn_batch_fetch_borders(dyn_batch* b, dyn_border_out* out);
/* (added within ABI 10) The posterior path samples of the batch's last align(calc_probabilities = 1) job, copied on the handle's
 * own non-blocking stream; out->count is set to the batch's K. DYN_ERR_INVALID_ARGUMENT (with a message) when the batch was
 * submitted with dyn_aligner_set_posterior_samples off, or was a Z-only or train job, or out's capacity, n or count is too small. */
int dyn_batch_fetch_samples(dyn_batch* b, dyn_sample_out* out);
/* (added within ABI 10) The credible intervals of the batch's last align(calc_probabilities = 1) job (of a completed ticket,
 * merged launch or not), copied on the handle's own non-blocking stream. DYN_ERR_INVALID_ARGUMENT (with a message) when the
 * batch was submitted with dyn_aligner_set_border_interval off, or aligned with calc_probabilities = 0, or out->capacity is too
 * small. */
int dyn_batch_fetch_intervals(dyn_batch* b, dyn_border_interval_out* out);
/* (added within ABI 10) The posterior-weighted per-base sums of the batch's last align(calc_probabilities = 1) job (of a
 * completed ticket, merged launch or not), copied on the handle's own non-blocking stream. DYN_ERR_INVALID_ARGUMENT (with a
 * message) when the batch was submitted with dyn_aligner_set_soft_levels off, or aligned with calc_probabilities = 0, or
 * out->capacity is too small. */
int dyn_batch_fetch_soft_levels(dyn_batch* b, dyn_soft_level_out* out);
/* (added within ABI 10) The site calls of the batch's last align(calc_probabilities = 1) job (of a completed ticket, merged launch
 * or not), copied on the handle's own non-blocking stream. DYN_ERR_INVALID_ARGUMENT (with a message) when the batch was submitted
 * with dyn_aligner_set_site_calls off, or aligned with calc_probabilities = 0, or out->capacity is too small. */
int dyn_batch_fetch_site_calls(dyn_batch* b, dyn_site_call_out* out);
/* (ABI 10) Copy the per-read transforms of the last dyn_batch_align (or of a completed ticket, merged launch or not) into
 * `out` (n >= the batch's read count). DYN_ERR_INVALID_ARGUMENT + message for a batch submitted with
 * dyn_aligner_set_rescale(a, 0), or aligned with calc_probabilities = 0. */
int dyn_batch_fetch_rescale(dyn_batch* b, dyn_rescale_out* out);
/* (added within ABI 10) The band margins of the batch's last align(calc_probabilities = 1) job (or of a completed ticket,
 * merged launch or not), copied on the handle's own non-blocking stream into `out` (n >= the batch's read count).
 * DYN_ERR_INVALID_ARGUMENT + message for a batch submitted with dyn_aligner_set_band_margin off, or aligned with
 * calc_probabilities = 0. */
int dyn_batch_fetch_band_margin(dyn_batch* b, dyn_band_margin_out* out);
/* (added within ABI 10) Guided band: the batch's next dyn_batch_align runs every ok read inside a window of `half_width`
 * lattice columns on either side of a per-sample guide path instead of the band around the fixed diagonal
 * (INTEGRATION.md section 3). centres[count]: one int32 per signal sample of the batch, read i's at the read's own signal
 * offset (sig_offsets[i] - sig_offsets[0]); centres of lattice row t >= 1 of a read = its entry t - 1, a lattice column of
 * 0 .. N - 1 (N = k-mers + 1), never decreasing along a read; row 0 is centred on column 0. half_width: 1 .. 2046, used as
 * given (not clamped to N / 2). The array is copied to the device before the call returns. A diagonal guide at
 * half_width = min(band / 2, N / 2) is the unguided band: same bits. A guide whose windows do not connect (0, 0) with
 * (T - 1, N - 1) costs that read DYN_READ_Z_MISMATCH and no other read anything; a read whose lattice of
 * 25 * T * (2 half_width + 3) bytes does not fit 0.8 of the free memory (or dyn_aligner_set_mem_budget) gets
 * DYN_READ_TOO_LARGE. For batches from dyn_batch_create / dyn_batch_create_raw that have not run yet (a batch created on a
 * DYN_DEVICE_HOST_ONLY handle is validated and nothing else). DYN_ERR_INVALID_ARGUMENT + a message that names the read and
 * the sample: count differs from the batch's samples, a centre outside [0, N - 1], a decreasing pair, half_width outside
 * [1, 2046], a batch that has already run, an asynchronous ticket. On a guided batch dyn_batch_train is refused (the guided
 * training job is a call of its own, dyn_batch_train_guided), and so is
 * dyn_batch_align while dyn_aligner_set_rescale(iters > 0) or dyn_aligner_set_border_confidence(window > 0) is on (both
 * DYN_ERR_INVALID_ARGUMENT + message); event stats, segment scores, the k-mer summary and the band margins (taken against
 * the guided window) work. dyn_batch_timing counts T * (2 half_width + 1) cells per read. */
int dyn_batch_set_guide(dyn_batch* b, const int32_t* centres, uint64_t count, uint32_t half_width);
/* (added within ABI 10) dyn_batch_train inside the guide that dyn_batch_set_guide put on the batch */
int dyn_batch_train_guided(dyn_batch* b);
/* The Baum-Welch statistics of every ok read over the cells of the guided window (the window of the guided dyn_batch_align,
 * INTEGRATION.md section 3): per lattice column the sums w, s1, s2 of g = exp(LPM) + exp(LPE), g x, (g x) x, each formed in
 * ascending row order without atomics (the same bits run to run, whatever the launch), and the transition counts N - 1 and
 * T - 1 - 2 (N - 1). Results are fetched as after dyn_batch_train (dyn_batch_fetch_train, dyn_batch_pooled_device). A read
 * whose guide is infeasible gets DYN_READ_TRAIN_Z_MISMATCH alone; a read whose 16 * T * (2 half_width + 3) bytes of lattice do
 * not fit gets DYN_READ_TOO_LARGE. DYN_ERR_INVALID_ARGUMENT + message: NULL, a batch without a guide, an asynchronous ticket.
 * dyn_aligner_set_rescale and dyn_aligner_set_border_confidence are align's switches and are ignored, as dyn_batch_train
 * ignores them. */
/* (added within ABI 10) Self-guided band: the library makes the batch's guide itself. A pre-pass kernel (k_auto_guide) runs a
 * forward max-plus sweep over every ok read, inside a window of `half_width` columns on either side of a centre that follows
 * the row's best cell, and installs the centres as the batch's guide exactly as dyn_batch_set_guide would (definition:
 * INTEGRATION.md section 3). The guide never decreases, lies in [0, N - 1] and connects the lattice's corners. half_width:
 * 1 .. 2046; it is also the half width of the batch's guided jobs. For batches from dyn_batch_create / dyn_batch_create_raw
 * that have not run yet. DYN_ERR_INVALID_ARGUMENT + message: half_width outside [1, 2046], an asynchronous ticket, a batch
 * that has already run; DYN_ERR_RUNTIME on a DYN_DEVICE_HOST_ONLY handle ("no GPU bound to this handle"). */
int dyn_batch_auto_guide(dyn_batch* b, uint32_t half_width);
/* (added within ABI 10) Guide refinement: the batch's next dyn_batch_align(b, 1) runs up to max_rounds alignments per read.
 * After an alignment, an ok read's called path becomes its next guide, g'[s] = the path's column at lattice row s + 1 (0
 * before the first border); where g' equals the guide in every entry the read has converged and its result stands, otherwise
 * it is aligned again inside g', at the same half width. Converged reads are not computed again. A read's status and outputs
 * are those of its last alignment; event stats, segment scores, band margins and the k-mer summary are computed once, after
 * that. max_rounds: 1 .. 64, 1 (the default) = one alignment and no comparison. DYN_ERR_INVALID_ARGUMENT + message:
 * max_rounds outside [1, 64], a batch without a guide, an asynchronous ticket. With max_rounds > 1 dyn_batch_align(b, 0) and
 * dyn_batch_train_guided are refused (neither has a called path). */
int dyn_batch_set_guide_refine(dyn_batch* b, uint32_t max_rounds);
/* (added within ABI 10) The batch's current guide, out[count] laid out as dyn_batch_set_guide's centres (count = the batch's
 * samples): what dyn_batch_set_guide or dyn_batch_auto_guide installed, and after a refined alignment every read's guide of
 * its last round. Entries of reads that failed validation: as set (0 after dyn_batch_auto_guide). */
int dyn_batch_fetch_guide(dyn_batch* b, int32_t* out, uint64_t count);
/* (added within ABI 10) Per read of a guided batch after dyn_batch_align(b, 1): rounds[i] = the alignments read i ran (0 for a
 * read that never reached the device), converged[i] = 1 where its last called path reproduced its guide (always 0 without
 * dyn_batch_set_guide_refine(max_rounds > 1)). n >= the batch's read count. */
int dyn_batch_fetch_guide_rounds(dyn_batch* b, uint32_t* rounds, uint32_t* converged, uint64_t n);
/* (added within ABI 10) The self-guided band for asynchronous tickets. While half_width > 0, every align ticket with
 * calc_probabilities = 1 (dyn_batch_align_async, dyn_batch_align_raw_async, dyn_batch_align_vbz_async) is aligned as a
 * synchronous batch is after dyn_batch_auto_guide(b, half_width) + dyn_batch_set_guide_refine(b, max_rounds): the same
 * status, Z, rows, rounds, converged flags and final guides, bit for bit. The switch is read when a ticket is submitted;
 * Z-only tickets, train tickets, synchronous batches and dyn_multi_* are untouched by it. Such a ticket is a launch of its
 * own: it is not merged with others and not published into the resident read queue (an open session is closed and waited
 * for first, as for a ticket that holds a wide read), and with max_rounds > 1 every read is refined inside that one launch,
 * by the workgroup that holds it. After dyn_batch_wait, dyn_batch_fetch_guide_rounds and dyn_batch_fetch_guide work on the
 * ticket; event stats, segment scores, the k-mer summary and the band margins (against the guided window) combine with it.
 * half_width 0 (the default): off, max_rounds is not looked at. Otherwise half_width in [1, 2046] and max_rounds in [1, 64]
 * (1 = the pre-pass and one alignment), else DYN_ERR_INVALID_ARGUMENT + message. A ticket submitted while the switch is on
 * together with dyn_aligner_set_rescale(iters > 0) or dyn_aligner_set_border_confidence(window > 0) is refused at submission
 * (DYN_ERR_INVALID_ARGUMENT + message), as dyn_batch_align refuses the pairing on a guided batch. */
int dyn_aligner_set_auto_guide(dyn_aligner* a, uint32_t half_width, uint32_t max_rounds);
/* (added within ABI 10) The guide rescue: self-guide only the reads whose band margin flags them. While half_width > 0, every
 * dyn_batch_align(b, 1) of a synchronous, unguided batch and every align ticket with calc_probabilities = 1 (the switch is read
 * when the job is started / the ticket is submitted)
 *   1. aligns every read exactly as without the switch (read queue, diagonal banded-lattice kernel);
 *   2. takes every read's band margins against the diagonal band, whether or not dyn_aligner_set_band_margin is on;
 *   3. flags a read when its status is ok, N >= 2 and min(margin_low, margin_high) < min_margin, a margin of
 *      DYN_BAND_MARGIN_NONE counting as +infinity;
 *   4. aligns the flagged reads again as a self-guided ticket aligns them (the pre-pass at half_width, then up to max_rounds
 *      alignments refined by the workgroup that holds the read): status, Z, rows, probabilities, rounds and converged of a
 *      rescued read are what dyn_batch_auto_guide(half_width) + dyn_batch_set_guide_refine(max_rounds) give for it;
 *   5. runs everything behind the traceback (segment rows, event stats, segment scores, k-mer summary) once, over all reads.
 * All of it happens on the device, in stream order, without a host round trip. Per read a code (dyn_batch_fetch_rescue):
 *   0 not flagged (a read the plain alignment failed included: such a read is NOT rescued), 1 rescued, 2 flagged but its
 *   lattice arena does not fit the memory the job may use (dyn_aligner_set_mem_budget), 3 flagged but the rescue alignment ended
 *   with a failure status; 2 and 3 keep the plain answer bit for bit.
 * With dyn_aligner_set_band_margin a code-1 read reports its margins against its guided window (as a guided batch does), every
 * other read against the diagonal. Z-only jobs, train jobs and dyn_multi_* ignore the switch. A ticket under the switch is a
 * launch of its own: not merged, not published into the resident read queue (an open session is closed and waited for first).
 * half_width 0 (the default): off. Otherwise half_width in [1, 2046], min_margin >= 0 (0 flags nothing) and max_rounds in
 * [1, 64], else DYN_ERR_INVALID_ARGUMENT + message. Refused with a message naming both when the job is started / the ticket is
 * submitted: together with dyn_aligner_set_rescale(iters > 0), dyn_aligner_set_border_confidence(window > 0) or
 * dyn_aligner_set_auto_guide(half_width > 0); on a batch that carries a guide (dyn_batch_set_guide / dyn_batch_auto_guide). */
int dyn_aligner_set_guide_rescue(dyn_aligner* a, int min_margin, uint32_t half_width, uint32_t max_rounds);
/* (added within ABI 10) Per read of a batch / a waited ticket whose last dyn_batch_align(b, 1) ran under
 * dyn_aligner_set_guide_rescue: code[i] as above; rounds[i] = the alignments the rescue ran for a code-1 read, converged[i] = 1
 * where its last called path reproduced its guide; both 0 for every other read. n >= the batch's read count.
 * DYN_ERR_INVALID_ARGUMENT + message for a batch that was not aligned under the switch. */
int dyn_batch_fetch_rescue(dyn_batch* b, uint8_t* code, uint32_t* rounds, uint32_t* converged, uint64_t n);
/* (added within ABI 10) Device bytes the batch's last job allocated for per-workgroup lattice arenas: workgroups x the largest
 * read's lattice, for the guided kernel (dyn_batch_set_guide) or the generic wide-band kernel (one kernel: band_reads.hip); 25 B per band slot
 * for align with probabilities, 16 B for dyn_batch_train / dyn_batch_train_guided; 0 for a batch whose reads all took the paged
 * read queue (its pool: dyn_timing.pool_pages) and for a Z-only job, guided or wide: it stores nothing of the lattice, so a wide
 * read is never DYN_READ_TOO_LARGE in a Z-only call. */
int dyn_batch_arena_bytes(const dyn_batch* b, uint64_t* bytes);
/* Device-resident results of the last dyn_batch_align, for an RCCL gather without a host hop:
 * rows = dyn_segment_row[capacity] (read i at seg_offsets[i], as in dyn_align_out);
 * z_status = per read {double Z; int32 status; uint32 n_segments}. Pointers stay valid until the
 * next call on the batch. */
int dyn_batch_device_results(dyn_batch* b, void** d_rows, uint64_t* capacity, void** d_z_status);
/* Device-resident pooled sufficient statistics (3*num_kmers doubles) of the last
 * dyn_batch_train, for an RCCL all-reduce. Computed by the first call (a sort by k-mer and a fixed-order sum of the
 * launch's per-column sums, on the handle's compute stream) and waited for: training that never asks does not pay for it. */
int dyn_batch_device_pooled(dyn_batch* b, void** d_pooled3n, uint64_t* count);
int dyn_batch_timing(const dyn_batch* b, dyn_timing* t);

/* Planning diagnostic, needs no GPU. A batch runs as ONE launch of persistent waves that take reads off a
 * queue; the lattice of a read lives in pages of a pool. When the pool cannot hold a lattice for every wave
 * (long reads: BASELINE config 3), the engine plans the queue order by replaying the launch on the host. This
 * entry exposes that planner: pages[i] / rows[i] = lattice pages and rows of read i, LONGEST FIRST; n_slots =
 * persistent waves (4 per CU); pool_pages = pages in the pool. order_out[k] = index of the read at queue position k;
 * the makespans are in lattice rows per wave (every wave sweeps rows at the same rate). */
int dyn_plan_queue(uint64_t n_reads, const uint32_t* pages, const uint64_t* rows, uint64_t n_slots,
                   uint64_t pool_pages, uint32_t* order_out, uint64_t* makespan_longest_first,
                   uint64_t* makespan_planned);
/* (ABI 6, additive) Planning diagnostic, needs no GPU: the order in which a PAGED session of the resident read queue takes
 * the reads of a page-starved ticket. Input: n_reads reads ranked LONGEST FIRST (rank 0 = longest); order_out[k] = rank of
 * the read at queue position k. The longer 7/8 are dealt out in a low-discrepancy order (any window of consecutive positions
 * holds ranks spread evenly over the whole range: the demand for lattice pages stays near its average), the shortest eighth
 * follows, longest first. */
int dyn_session_order(uint64_t n_reads, uint32_t* order_out);

/* ---- asynchronous form: a stream of batches with H2D, kernels, D2H and host marshalling of
 * neighbouring batches overlapped (the reference keeps its worker pool permanently fed,
 * segment.py:301-325) ----
 *
 * dyn_batch_align_async == dyn_align_batch, but returns at once with a ticket: validateInput /
 * sequenceToKmers, the H2D copy, every kernel, the D2H copy and the unpacking into `out` run on the
 * handle's pipeline threads and streams. Batches of one handle complete in submission order.
 * EVERYTHING the call was given (signals, offsets, seqs, `out` and the arrays it points to) must stay
 * valid and untouched until dyn_batch_wait(ticket) has returned. After the wait the ticket behaves
 * like an aligned batch: dyn_batch_timing and dyn_batch_device_results work on it. Release it with
 * dyn_batch_destroy (which waits first if need be). Inputs allocated with dyn_host_alloc are copied
 * by DMA without staging.
 * Merged launches: a read-queue launch of fewer reads than the device has waves (1 024) cannot balance -- every wave
 * holds one read and the launch lasts as long as its slowest. Align tickets of one kind that are WAITING while the GPU
 * still has a launch queued are therefore run as one launch (at most a quarter of the tickets the caller has had in
 * flight at once -- 12 in flight: launches of three batches -- and eight reads per wave): same results, same
 * completion order, and each ticket still reports the launch that carried it (dyn_timing, launch_share) and serves its
 * own slice of the device rows (dyn_batch_device_results). A ticket that finds the GPU idle starts at once, alone;
 * training tickets are never merged. Environment variable DYN_NO_MERGE=1 switches the merging off. */
int dyn_batch_align_async(dyn_aligner* a, uint64_t n_reads, const double* signals,
                          const uint64_t* sig_offsets, const char* seqs, const uint64_t* seq_offsets,
                          int calc_probabilities, dyn_align_out* out, dyn_batch** ticket);
/* dyn_train_batch in the same form (pooled3n as there; it is accumulated into when the batch completes). */
int dyn_batch_train_async(dyn_aligner* a, uint64_t n_reads, const double* signals,
                          const uint64_t* sig_offsets, const char* seqs, const uint64_t* seq_offsets,
                          dyn_train_out* out, double* pooled3n, dyn_batch** ticket);
/* The asynchronous calls on RAW slices: dyn_batch_create_raw's preprocessing (P1/P2: segment.py:146-153,
 * train.py:163-170, utils.py:16-43) as the first stage of the same pipeline -- the helper threads gather
 * [offsets | shift | scale | samples] into pinned staging, one DMA carries them up, k_normalise / k_hampel run on the
 * compute stream in front of the batch's read queue. This is what dynamont-resquiggle / dynamont-train drive: the
 * reference keeps its workers fed the same way (segment.py:296-325). raw_dtype 3 (these two calls only): int16 ADC
 * counts with the read's pod5 calibration, picoampere = (float(adc) + cal_offset[i]) * cal_scale[i] in float32 -- the
 * value `signal_pa` (src/dynamont/pod5_io.py:6-16) hands the reference, formed on the device instead (half the bytes
 * over PCIe, no per-read NumPy pass); cal_offset / cal_scale may be NULL for the other dtypes. raw, raw_offsets,
 * cal_*, shift, scale, seqs, seq_offsets and `out` must stay valid until dyn_batch_wait(ticket) has returned. */
int dyn_batch_align_raw_async(dyn_aligner* a, uint64_t n_reads, const void* raw, int raw_dtype,
                              const uint64_t* raw_offsets, const float* cal_offset, const float* cal_scale,
                              const double* shift, const double* scale,
                              int hampel_window, double hampel_n_sigmas, int compute_f32, const char* seqs,
                              const uint64_t* seq_offsets, int calc_probabilities, dyn_align_out* out,
                              dyn_batch** ticket);
int dyn_batch_train_raw_async(dyn_aligner* a, uint64_t n_reads, const void* raw, int raw_dtype,
                              const uint64_t* raw_offsets, const float* cal_offset, const float* cal_scale,
                              const double* shift, const double* scale,
                              int hampel_window, double hampel_n_sigmas, int compute_f32, const char* seqs,
                              const uint64_t* seq_offsets, dyn_train_out* out, double* pooled3n,
                              dyn_batch** ticket);
/* The same for a batch whose signal is still in POD5 form: VBZ-compressed chunks (POD5 format specification: zstd around
 * StreamVByte-16 of the zigzag-coded sample deltas) -- the decode ONT's pod5 library performs inside `record.signal`,
 * which the reference calls per read (src/dynamont/pod5_io.py:6-16). Read i's signal is the concatenation of the chunks
 * [read_chunk_offsets[i], read_chunk_offsets[i+1]) (chunk c: chunk_bytes[c] compressed bytes at chunk_ptrs[c] holding
 * chunk_samples[c] samples), of which the slice [slice_start[i], slice_start[i] + (raw_offsets[i+1] - raw_offsets[i]))
 * is aligned (segment.py:147: signal[start:end]). The pipeline's helper threads decode whole reads straight into the
 * pinned staging buffer. cal_offset / cal_scale as for raw_dtype 3, or both NULL for plain ADC counts (raw_dtype 1).
 * A chunk that does not decode fails the batch with DYN_ERR_RUNTIME ("VBZ: ..."). */
int dyn_batch_align_vbz_async(dyn_aligner* a, uint64_t n_reads, const void* const* chunk_ptrs, const uint64_t* chunk_bytes,
                              const uint32_t* chunk_samples, const uint64_t* read_chunk_offsets, const uint64_t* slice_start,
                              const uint64_t* raw_offsets, const float* cal_offset, const float* cal_scale,
                              const double* shift, const double* scale, int hampel_window, double hampel_n_sigmas,
                              int compute_f32, const char* seqs, const uint64_t* seq_offsets, int calc_probabilities,
                              dyn_align_out* out, dyn_batch** ticket);
/* One VBZ chunk -> `samples` int16 values (host only; tests, other readers). */
int dyn_vbz_decode(const void* blob, uint64_t blob_bytes, uint32_t samples, int16_t* out, char* err, uint64_t errcap);
/* Block until the batch behind the ticket is complete; returns its status code, with the message in
 * dyn_aligner_last_error. Returns DYN_OK at once for batches of the synchronous calls. */
int dyn_batch_wait(dyn_batch* ticket);
/* Page-locked host memory for inputs/outputs of the asynchronous calls (NULL on failure). */
void* dyn_host_alloc(uint64_t bytes);
void dyn_host_free(void* p);

/* ---- several GPUs behind one handle (reads are independent, NT_aligner_api.cpp:230-312) ----
 *
 * dyn_multi owns one dyn_aligner per entry of device_ids (an ordinal may appear more than once). A batch is cut
 * into n_devices contiguous ranges of equal lattice work (sum of signal lengths); every range runs through its
 * device's asynchronous pipeline and the results land directly in the caller's arrays, in the layout of
 * dyn_align_batch / dyn_train_batch. No device-to-device traffic and no Python: this is how a C/C++ host shards
 * a batch over the GPUs of a node (one PROCESS per GPU with an RCCL gather is the other form: bench.py --gpus N). */
int dyn_multi_create(const char* model_path, int pore, const char* mode, int threads, uint64_t band,
                     const int* device_ids, int n_devices, dyn_multi** out, char* err, uint64_t errcap);
void dyn_multi_destroy(dyn_multi* m);
int dyn_multi_device_count(const dyn_multi* m);
/* the per-device handle (dyn_aligner_info, dyn_aligner_model, dyn_aligner_set_mem_budget, dyn_aligner_set_rescale, ...) */
dyn_aligner* dyn_multi_handle(dyn_multi* m, int i);
const char* dyn_multi_last_error(const dyn_multi* m);
int dyn_multi_align_batch(dyn_multi* m, uint64_t n_reads, const double* signals, const uint64_t* sig_offsets,
                          const char* seqs, const uint64_t* seq_offsets, int calc_probabilities, dyn_align_out* out);
/* pooled3n as in dyn_train_batch: the sum over all devices is ADDED to it */
int dyn_multi_train_batch(dyn_multi* m, uint64_t n_reads, const double* signals, const uint64_t* sig_offsets,
                          const char* seqs, const uint64_t* seq_offsets, dyn_train_out* out, double* pooled3n);

/* ---- one PROCESS per GPU: the two exchanges of a multi-GPU job over RCCL / xGMI ----
 *
 * The reference scales by forking worker processes on one host (segment.py:296-325); reads are independent
 * (NT_aligner_api.cpp:230-312), so a multi-GPU job shards the reads over one process per GPU and needs nothing but
 *   config 4: a gather of the per-read segment rows to one rank           -> dyn_comm_gather_rows
 *   config 5: a sum all-reduce of the pooled statistics (w, s1, s2)[4^k]  -> dyn_comm_allreduce_pooled
 * both straight from the device buffers of a batch. librccl is bound with dlopen at the first call below; nothing else
 * in this library needs it. Rank 0 creates the 128-byte id and hands it to the other ranks by the host's own means
 * (a file, MPI, a socket); dyn_comm_create is collective (ncclCommInitRank). One communicator per process and GPU. */
#define DYN_COMM_ID_BYTES 128
typedef struct dyn_comm dyn_comm;
int dyn_comm_unique_id(uint8_t* id_out128, char* err, uint64_t errcap);
int dyn_comm_create(const uint8_t* id128, int rank, int n_ranks, int device, dyn_comm** out, char* err, uint64_t errcap);
void dyn_comm_destroy(dyn_comm* c);
const char* dyn_comm_last_error(const dyn_comm* c);
/* The gather of config 4 is two collectives: the 8-byte count exchange, then the rows.
 * dyn_comm_gather_counts: collective. `b` = an aligned batch or a ticket of dyn_batch_align[_raw]_async (waited for
 * here). counts_out[r] (n_ranks entries, may be NULL) = the dyn_segment_row records rank r will send
 * (dyn_segment_capacity() of its batch). A rank whose batch FAILED announces 0 rows, takes part in both collectives all
 * the same -- its peers never block on it -- and gets its batch's error code back from both calls.
 * dyn_comm_gather_rows: collective. The rows travel device to device to `root`: one ncclSend per peer, each over its own
 * xGMI link, no padding. On root rows_out (host, may be NULL; rows_cap records) receives them back to back in rank order
 * (read i of a rank at seg_offsets[i] as in dyn_align_out). Called without a preceding dyn_comm_gather_counts it performs
 * the count exchange itself; a root that cannot know the total in advance calls dyn_comm_gather_counts first and
 * allocates sum(counts). rows_cap < total on root: the exchange completes on every rank (nothing hangs), the rows are
 * dropped and root gets DYN_ERR_INVALID_ARGUMENT.
 * A HIP / RCCL failure in the middle of an exchange aborts the communicator (ncclCommAbort), and so does an exchange that is
 * not complete after DYN_COMM_TIMEOUT_S seconds (default 300; a peer that died or never arrived -- RCCL's kernels wait for
 * their peers on the device, so the wait is a polled one): the call fails with DYN_ERR_DEVICE, every later call on the
 * handle returns DYN_ERR_DEVICE at once. */
int dyn_comm_gather_counts(dyn_comm* c, dyn_batch* b, uint64_t* counts_out);
int dyn_comm_gather_rows(dyn_comm* c, dyn_batch* b, int root, dyn_segment_row* rows_out, uint64_t rows_cap,
                         uint64_t* counts_out);
/* Collective. `b` = a trained batch or a ticket of dyn_batch_train[_raw]_async. Sum over ranks of the device-resident
 * pooled statistics (dyn_batch_device_pooled; reduced in place), copied to pooled3n (3 * num_kmers doubles, may be NULL). */
int dyn_comm_allreduce_pooled(dyn_comm* c, dyn_batch* b, double* pooled3n);
/* (ABI 7, additive) The same exchange for payloads that live in HOST memory -- what the multi-rank CLIs move: a rank's part
 * of the compressed output frame and its `.errors` lines to rank 0 (the reference's listener collects every worker's rows,
 * src/dynamont/segmentation/segment.py:296-325,69-107), the training loop's per-batch sums (train.py:195-220 over all ranks).
 * dyn_comm_gather_bytes: collective. n_bytes of `bytes` from every rank to `root` through the code path of
 * dyn_comm_gather_rows (8-byte count all-gather, then one ncclSend per peer / ncclRecv per peer on the root in one group;
 * the payload is staged on the device first). counts_out[r] (n_ranks entries, may be NULL) = rank r's n_bytes, on every rank.
 * On root the gathered bytes stay in the communicator's device buffer until the next gather:
 * dyn_comm_gathered_bytes copies them out, back to back in rank order (out_cap >= sum of the counts; not a collective).
 * dyn_comm_allreduce_f64: collective. Elementwise over ranks, in place on the caller's n doubles; op 0 = sum, 1 = max.
 * Bounded like every exchange here: DYN_COMM_TIMEOUT_S (default 300) seconds or an asynchronous RCCL error abort the
 * communicator and fail the call -- a peer that has gone costs its peers an error, not a hang. */
int dyn_comm_gather_bytes(dyn_comm* c, const void* bytes, uint64_t n_bytes, int root, uint64_t* counts_out);
int dyn_comm_gathered_bytes(dyn_comm* c, void* out, uint64_t out_cap);
int dyn_comm_allreduce_f64(dyn_comm* c, double* inout, uint64_t n, int op);

#ifdef __cplusplus
}
#endif
#endif /* DYNAMONT_MI_H */
