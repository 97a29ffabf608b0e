// guided_band_kernels.hpp -- launch interface of the guided band (guided_band.hip, dyn_batch_set_guide): the lattice of a read
// is banded around a per-sample guide path instead of the fixed diagonal mid(t) = int(t * N / T).
//
// Window. For lattice row t >= 1 the centre is centre(t) = guide[sig_off + t - 1] (one int32 per
// signal sample, at the read's own signal offset), centre(0) = 0; bw is the batch's half width, NOT clamped to N / 2;
// B = 2 bw + 3 band columns per row incl. the two guards; start_t = centre(t) - bw; band column c <-> lattice column
// n = start_t + c - 1; the cells of row t are n in [max(start_t, 1 or 0), min(centre(t) + bw + 1, N)) -- the reference's
// computeBounds (NT_aligner_api.cpp:90-108) with mid -> centre. The shift between neighbouring rows, start_t - start_{t-1},
// is >= 0 (the guide is non-decreasing: validated on the host) and of any size.
#pragma once

#include "nt_kernels.hpp"

namespace dynk {

struct GuidedArgs {
  const ReadDesc* descs;   // every ok read of the batch (ReadDesc::bw is not used: the half width is the launch's)
  int n_reads;
  int bw;                  // half width, 1 .. WIDE_MAX_HALF_BAND
  const double* sig;
  const Emis* par;
  const int32_t* guide;    // [samples of the batch]: ReadDesc::sig_off counts from here, as it does into sig
  ReadState* st;
  TraceBuffers tb;
  TrainBuffers tr;         // job 2 only: the read's column sums at col_* + ReadDesc::par_off, trans[2 * read]
  char* arena;             // n_groups arenas of arena_bytes: the lattice of the read a workgroup is working on (jobs 1 and 2)
  uint64_t arena_bytes;    // >= guided_arena_bytes of the largest read
  uint32_t* head;          // queue head (cleared by launch_guided_reads)
  const uint64_t* exp_tab; // dynmath::strict_exp_table on the device
  double m1, e2;
  int z_fail_status;
  // a refinement round (dyn_batch_set_guide_refine): the reads to align are descs[active[0 .. *n_active)], list and length
  // written on the device by launch_guide_refine. Null: every descriptor
  const uint32_t* active;
  const uint32_t* n_active;
};

// one step of the guide refinement, behind a launch_guided_reads(job 1) over the same descriptors
struct GuideRefine {
  const ReadDesc* descs;
  int n_reads;
  const ReadState* st;
  const uint32_t* pathn;      // TraceBuffers::pathn
  const uint32_t* segrow;     // TraceBuffers::segrow
  int32_t* guide;             // the batch's guide: rewritten for the reads that go on
  uint32_t* rounds;           // [reads of the batch] alignments run so far (+1 for every read of active_in)
  uint32_t* converged;        // [reads of the batch] set to 1 where the called path reproduces the guide
  const uint32_t* active_in;  // the reads the launch before this step aligned, and their number (null: every descriptor)
  const uint32_t* n_in;
  uint32_t* active_out;       // [n_reads] the reads of the next launch, and their number (cleared by launch_guide_refine)
  uint32_t* n_out;
  int last;                   // the last round: compare only, the guide stays the one the last alignment used
};
hipError_t launch_guide_refine(const GuideRefine& r, hipStream_t s);

// bytes of lattice one workgroup needs for a read of T rows: 25 B per band slot with probabilities (bE, bM doubles; float LPM,
// float LPE; one decision byte), 16 B for the train job (bE, bM), nothing for the Z-only job (its backward rows never leave
// LDS). job as launch_guided_reads takes it.
uint64_t guided_arena_bytes(uint64_t T, uint64_t bw, int job);
// the most workgroups per compute unit the shape chosen for this half width is launched with (an upper bound: it limits the
// arenas a launch allocates)
int guided_groups_per_cu(int bw, int job);
// job: 0 = Z only, 1 = align(calc_probabilities = true) up to the per-row path arrays (launch_segments follows), 2 = train:
// the read's (w, s1, s2) column sums and transition counts in GuidedArgs::tr (finalise_train / pool_stats follow). Returns what
// raising the dynamic-LDS limit (windows above 48 KiB of rows) or the launch reported.
hipError_t launch_guided_reads(int job, const GuidedArgs& a, int n_groups, hipStream_t s);

// band margins of a guided batch: INTEGRATION.md section 3's definition with mid(t) -> centre(t), bw -> half width, over the
// path rows [segrow[0], T). rows_total: the batch's path rows (sum of T over descs).
void launch_guided_band_margin(const ReadDesc* descs, int n_reads, uint32_t max_T, const ReadState* st, const TraceBuffers& tb,
                               const int32_t* guide, int bw, const BandMargin& bm, hipStream_t s);

}  // namespace dynk
