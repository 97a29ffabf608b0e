// band_margin.hip -- band-margin diagnostics (dyn_aligner_set_band_margin): per read, how close the called path came to a real
// edge of its band. The kernels and the definition are in band_margin_kernels.hpp (shared with
// tests/device_math/band_margin.hip).
#include "band_margin_kernels.hpp"

namespace dynk {

void launch_band_margin(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                        const BandMargin& bm, hipStream_t s) {
  launch_band_margin_kernels(descs, n_reads, max_N, st, tb.segrow, bm, s);
}

}  // namespace dynk
