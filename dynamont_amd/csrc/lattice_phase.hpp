// lattice_phase.hpp -- the lattice phases: the opt-in outputs that read a read's lattice while it is still in place, behind
// the read in k_read_queue (nt_kernels.hip) and in the diagonal k_band_reads (band_reads.hip). Which of them a launch carries
// is decided HERE, once, for both kernels. No HIP header: the host tests compile it with g++ (tests/test_lattice_phase_host.py).
#pragma once

namespace dynk {

// Bits on top of JOB_ALIGN / JOB_ALIGN_INPLACE in k_read_queue's template argument, and k_band_reads' PHASES.
constexpr int JOB_BORDER = 8;     // border confidence (border_kernels.hpp)
constexpr int JOB_SAMPLE = 16;    // posterior samples (sample_kernels.hpp); behind the border phase when both bits are set
constexpr int JOB_INTERVAL = 32;  // credible intervals (interval_kernels.hpp); always alone
constexpr int JOB_SOFT = 64;      // soft levels (soft_level_kernels.hpp); always alone
constexpr int LATTICE_PHASE_BITS = JOB_BORDER | JOB_SAMPLE | JOB_INTERVAL | JOB_SOFT;

// SoftOut::tag (nt_kernels.hpp) when the soft levels are asked for: a value no sample count (0 .. 64) ever is
constexpr int SOFT_TAG = -1;

// The sets of phases a launch may carry: one kernel of either kind is instantiated for each, and for no other.
constexpr int LATTICE_PHASE_SETS[] = {0, JOB_BORDER, JOB_SAMPLE, JOB_SAMPLE | JOB_BORDER, JOB_INTERVAL, JOB_SOFT};
constexpr int N_LATTICE_PHASE_SETS = sizeof(LATTICE_PHASE_SETS) / sizeof(LATTICE_PHASE_SETS[0]);

// The phases of a launch. align_calc: the job is align(calc_probabilities=true) -- no other job keeps a lattice with posteriors.
// tag_word: the one word the three members of the union in QueueArgs / BandArgs share, SampleOut::count = IntervalOut::none =
// SoftOut::tag. tail: IntervalOut::tail. border_window: QueueArgs / BandArgs::border_window. A row per output:
constexpr int lattice_phases(bool align_calc, int tag_word, double tail, int border_window) {
  if (!align_calc) return 0;
  if (tag_word == SOFT_TAG) return JOB_SOFT;                                        // dyn_aligner_set_soft_levels
  if (tag_word == 0 && tail > 0.0) return JOB_INTERVAL;                             // dyn_aligner_set_border_interval
  if (tag_word > 0) return JOB_SAMPLE | (border_window > 0 ? JOB_BORDER : 0);       // dyn_aligner_set_posterior_samples
  return border_window > 0 ? JOB_BORDER : 0;                                        // dyn_aligner_set_border_confidence
}

}  // namespace dynk
