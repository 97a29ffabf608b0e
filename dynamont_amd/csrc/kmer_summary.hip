// kmer_summary.hip -- per-k-mer level summary of a run (dyn_aligner_set_kmer_summary): what level and dwell the run showed
// for every k-mer against what the model says, accumulated on the handle as exact integers while the switch is on. The
// kernels and the definition are in kmer_summary_kernels.hpp (shared with tests/device_math/kmer_summary.hip).
#include "kmer_summary_kernels.hpp"

namespace dynk {

void launch_kmer_summary(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                         const KmerSummary& ks, hipStream_t s) {
  launch_kmer_summary_kernels(descs, n_reads, max_N, st, tb.segrow, ks, s);
}

}  // namespace dynk
