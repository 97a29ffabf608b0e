// site_summary.hip -- per-site level summary of a run (dyn_aligner_set_site_summary): coverage, dwell and the sums of the
// reads' event means per caller-supplied site id, accumulated on the handle as exact integers while the switch is on. The
// kernels and the definition are in site_summary_kernels.hpp (shared with tests/device_math/site_summary.hip).
#include "site_call_kernels.hpp"
#include "site_compare_kernels.hpp"
#include "site_map_kernels.hpp"
#include "site_mixture_kernels.hpp"
#include "site_pack_kernels.hpp"
#include "site_quantile_kernels.hpp"
#include "site_summary_kernels.hpp"

namespace dynk {

void launch_site_summary(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                         const SiteSummary& ss, hipStream_t s) {
  launch_site_summary_kernels(descs, n_reads, max_N, st, tb.segrow, ss, s);
}

// dyn_aligner_site_quantiles: one window of the level histograms into its staging buffer
void launch_site_quantiles(const SiteQuantiles& sq, hipStream_t s) { launch_site_quantiles_kernel(sq, s); }

// dyn_aligner_site_compare: one window of site pairs into its staging buffer
void launch_site_compare(const SiteCompare& sc, hipStream_t s) { launch_site_compare_kernel(sc, s); }

// dyn_aligner_site_mixture: one window of site pairs into its staging buffer
void launch_site_mixture(const SiteMixture& sm, hipStream_t s) { launch_site_mixture_kernel(sm, s); }

// dyn_aligner_site_summary_add: one staged window into the table and its counters
void launch_site_add(const SiteAdd& sa, hipStream_t s) { launch_site_add_kernel(sa, s); }

// the window calls of a sparse table: one window of ids gathered into a dense scratch, one staged window scattered into the
// rows of its ids, the bitmap of the occupied id windows
void launch_site_gather(const SiteGather& sg, hipStream_t s) { launch_site_gather_kernel(sg, s); }
void launch_site_scatter_add(const SiteScatter& sc, hipStream_t s) { launch_site_scatter_add_kernel(sc, s); }
void launch_site_map_windows(const SiteWindows& sw, hipStream_t s) { launch_site_map_windows_kernel(sw, s); }

// dyn_aligner_site_pack / dyn_aligner_site_summary_merge: the live rows of a window of table rows as records (count and scan,
// then the write), and records added into the table by key
void launch_site_pack(const SitePack& sp, hipStream_t s) { launch_site_pack_kernels(sp, s); }
void launch_site_pack_write(const SitePack& sp, hipStream_t s) { launch_site_pack_write_kernel(sp, s); }
void launch_site_merge(const SiteMerge& sm, hipStream_t s) { launch_site_merge_kernel(sm, s); }

// dyn_aligner_set_site_calls: the rows of the reads [read_lo, read_hi) scored against the per-site model (site_call_kernels.hpp),
// and the model's two window calls on a sparse table
void launch_site_calls(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const TraceBuffers& tb,
                       const SiteCalls& sc, hipStream_t s) {
  launch_site_call_kernels(descs, n_reads, max_N, st, tb.segrow, sc, s);
}
void launch_site_model_scatter(const SiteModelScatter& ms, hipStream_t s) { launch_site_model_scatter_kernel(ms, s); }
void launch_site_model_gather(const SiteModelGather& mg, hipStream_t s) { launch_site_model_gather_kernel(mg, s); }

}  // namespace dynk
