// segment_scores.hip -- per-border segment quality scores (dyn_aligner_set_segment_scores): the kernels and their definition
// are in segment_score_kernels.hpp, which tests/device_math/segment_scores.hip includes as well.
#include "segment_score_kernels.hpp"

namespace dynk {

void launch_segment_scores(const ReadDesc* descs, int n_reads, uint64_t rows_total, uint32_t max_N, const ReadState* st,
                           const TraceBuffers& tb, const ScoreCols& sc, hipStream_t s) {
  launch_segment_score_kernels(descs, n_reads, rows_total, max_N, st, tb.pathn, tb.segrow, sc, s);
}

}  // namespace dynk
