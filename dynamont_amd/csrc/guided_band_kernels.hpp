// guided_band_kernels.hpp -- launch interface of what a guided batch (dyn_batch_set_guide) runs beside the banded-lattice kernel
// (band_reads.hpp, GuideWindow: the lattice of a read is banded around a per-sample guide path instead of the fixed diagonal
// mid(t) = int(t * N / T)): the guide refinement and the band margins against the guide's window (guided_band.hip).
#pragma once

#include "nt_kernels.hpp"

namespace dynk {

// one step of the guide refinement, behind a launch_band_reads(job 1) over the same descriptors
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

// band margins of a guided batch: INTEGRATION.md section 3's definition with mid(t) -> centre(t), bw -> half width, over the
// path rows [segrow[0], T). rows_total: the batch's path rows (sum of T over descs).
// only: a per-read code, [reads of the batch] (the guide rescue's, guide_rescue_kernels.hpp): the margins of the reads whose code
// is 1 are taken against the guide's window, every other read's entries are left as they are. Null: every read of bm's range.
void launch_guided_band_margin(const ReadDesc* descs, int n_reads, uint32_t max_T, const ReadState* st, const TraceBuffers& tb,
                               const int32_t* guide, int bw, const BandMargin& bm, hipStream_t s, const uint8_t* only = nullptr);

}  // namespace dynk
