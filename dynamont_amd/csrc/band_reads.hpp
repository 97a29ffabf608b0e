// band_reads.hpp -- launch interface of the banded-lattice kernel (band_reads.hip): the reference's algorithm in its own
// band-column addressing, one workgroup per read, for the reads the register sweeps of nt_kernels.hip do not take -- the wide
// band (half band above MAX_HALF_BAND) and the guided band (dyn_batch_set_guide). One kernel body; what differs between the
// two is the WINDOW of a lattice row, a policy the body is instantiated with.
//
// Window. A row t has B = 2 bw + 3 band columns incl. the two guards; start_t = centre(t) - bw; band column c <-> lattice
// column n = start_t + c - 1; the cells of row t are n in [max(start_t, 1 or 0), min(centre(t) + bw + 1, N)) -- the reference's
// computeBounds (NT_aligner_api.cpp:90-108).
//   DiagonalWindow  (BandArgs::guide == nullptr) the reference's band: centre(t) = size_t(t * RATIO) (:100), bw = the read's own
//                   ReadDesc::bw = min(band / 2, N / 2); the shift between neighbouring rows is 0 or 1; the backward seed, Zb
//                   and Zf are read at the fixed band column bw + 1 (:170, :285-286). A launch holds reads of different B.
//   GuideWindow      centre(t) = guide[sig_off + t - 1] (one int32 per signal sample, at the read's
//                   own signal offset), centre(0) = 0; bw = BandArgs::bw, the batch's half width, NOT clamped to N / 2; the
//                   shift start_t - start_{t-1} is >= 0 (the guide is non-decreasing: validated on the host) and of any size;
//                   the backward seed and Zf are read at the band column of (T-1, N-1), and a read whose windows do not connect
//                   (0, 0) with it fails the reference's own Z check.
//   LiveGuideWindow (BandArgs::refine_rounds > 1) GuideWindow's geometry for the launch that rewrites a read's guide between two
//                   alignments of it: the centre is loaded so that the rewrite is seen (band_reads.hip).
#pragma once

#include "nt_kernels.hpp"

namespace dynk {

struct BandArgs {
  const ReadDesc* descs;   // the reads of the launch
  int n_reads;
  int bw;                  // guided: the half width, 1 .. WIDE_MAX_HALF_BAND (ReadDesc::bw is not used). Diagonal: not used
  const double* sig;
  const Emis* par;
  int32_t* guide;          // [samples of the batch]: ReadDesc::sig_off counts from here, as it does into sig. Null: the diagonal window.
                           // Read only, except by a refining launch (refine_rounds > 1), which rewrites it
  ReadState* st;
  TraceBuffers tb;
  union {                  // (as in QueueArgs: the two never meet, and the argument layout stays what it was)
    TrainBuffers tr;       // job 2 only: the read's column sums at col_* + ReadDesc::par_off, trans[2 * read]
    SampleOut sample;      // job 1 only, diagonal window, with or without a border window: posterior path samples, count > 0 when asked for
    IntervalOut interval;  // job 1 only, diagonal window, no border window: credible intervals, tail > 0 (and sample.count == 0) when asked for
    SoftOut soft;          // job 1 only, diagonal window, no border window: posterior-weighted per-base sums, tag == SOFT_TAG when asked for
  };
  char* arena;             // n_groups arenas of arena_bytes: the lattice of the read a workgroup is working on (jobs 1 and 2)
  uint64_t arena_bytes;    // >= band_arena_bytes of the largest read
  uint32_t* head;          // queue head (cleared by launch_band_reads)
  const uint64_t* exp_tab; // dynmath::strict_exp_table on the device
  double m1, e2;
  int z_fail_status;
  // a refinement round (dyn_batch_set_guide_refine) or the guide rescue (dyn_aligner_set_guide_rescue): the reads to align are
  // descs[active[0 .. *n_active)], list and length written on the device by launch_guide_refine / launch_rescue_select.
  // Null: every descriptor
  const uint32_t* active;
  const uint32_t* n_active;
  int border_window = 0;   // as QueueArgs: W, and the two columns of dyn_aligner_set_border_confidence (diagonal, job 1 only)
  double* border_p = nullptr;
  double* border_window_p = nullptr;
  // per-read refinement INSIDE the launch (guided, job 1, no border window): the workgroup that holds a read aligns it up to
  // refine_rounds times, each time inside the path the alignment before called, by the rules of launch_guide_refine
  // (guided_band_kernels.hpp) -- the round scheme's results bit for bit in one launch. 0 or 1: no refinement. Such a launch
  // honours active / n_active like any other (the guide rescue's list; a self-guided ticket passes none)
  int refine_rounds = 0;
  uint32_t* rounds = nullptr;     // [reads of the batch] alignments run, written for every read of the launch (cleared by the caller)
  uint32_t* converged = nullptr;  // [reads of the batch] set to 1 where the called path reproduces the guide (cleared by the caller)
};

// bytes of lattice one workgroup needs for a read of T rows: 25 B per band slot with probabilities (bE, bM doubles; float LPM,
// float LPE; one decision byte), 16 B for the train job (bE, bM), nothing for the Z-only job (its backward rows never leave
// LDS). job as launch_band_reads takes it.
uint64_t band_arena_bytes(uint64_t T, uint64_t bw, int job);
// the most workgroups per compute unit a launch is given (an upper bound: it limits the arenas a launch allocates). Diagonal
// (guided == false): 1, bw is not looked at; guided: what the shape chosen for this half width holds beside each other
int band_groups_per_cu(bool guided, int bw, int job);
// job: 0 = Z only, 1 = align(calc_probabilities = true) up to the per-row path arrays (launch_segments follows), 2 = train:
// the read's (w, s1, s2) column sums and transition counts in BandArgs::tr (finalise_train / pool_stats follow). Returns what
// raising the dynamic-LDS limit (guided rows above 48 KiB) or the launch reported. hipErrorInvalidValue for a refining launch
// (BandArgs::refine_rounds > 1) without a guide, with a job other than 1, with a border window or without rounds / converged,
// for posterior samples (BandArgs::sample.count > 0) with a guide, a job other than 1 or without their arrays, and for credible
// intervals (BandArgs::interval.tail > 0) with a guide, a border window or without their buffer, and likewise for the soft levels
// (BandArgs::soft.tag == SOFT_TAG). Which lattice phases a launch carries: lattice_phases() (lattice_phase.hpp), as for the read queue.
hipError_t launch_band_reads(int job, const BandArgs& a, int n_groups, hipStream_t s);

}  // namespace dynk
