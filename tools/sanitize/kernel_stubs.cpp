// Sanitizer builds of the HOST side (tools/sanitize/Makefile): the .hip translation units cannot be compiled by g++, and
// nothing in a CPU-only run may reach them -- every entry point of the device code is a stub that aborts loudly.
#include <cstdio>
#include <cstdlib>

#include "../../dynamont_amd/csrc/nt_kernels.hpp"
#include "../../dynamont_amd/csrc/band_reads.hpp"
#include "../../dynamont_amd/csrc/guided_band_kernels.hpp"
#include "../../dynamont_amd/csrc/auto_guide_kernels.hpp"
#include "../../dynamont_amd/csrc/guide_rescue_kernels.hpp"

namespace dynk {

[[noreturn]] static void no_device(const char* what) {
  std::fprintf(stderr, "sanitizer build: %s needs the GPU build of the library\n", what);
  std::abort();
}

void launch_session(bool, int, const SessionArgs&, const void*, void*, const dynmath::SoftplusNode*, int, hipStream_t) { no_device("launch_session"); }
void launch_session_publish(SessionTicket*, uint32_t*, const SessionTicket&, uint32_t, uint32_t, hipStream_t) { no_device("launch_session_publish"); }
void launch_session_close(uint32_t*, hipStream_t) { no_device("launch_session_close"); }
void launch_preprocess(const void*, int, int, const uint64_t*, const double*, const double*, const float*, const float*, void*, double*, int, uint64_t,
                       int, double, hipStream_t) {
  no_device("launch_preprocess");
}
void launch_prep_params(const int32_t*, const Emis*, Emis*, uint64_t, uint32_t, hipStream_t) { no_device("launch_prep_params"); }
void launch_pool_init(const PagePool&, uint32_t, int, hipStream_t) { no_device("launch_pool_init"); }
hipError_t launch_read_queue(QueueJob, bool, const QueueArgs&, int, hipStream_t) { no_device("launch_read_queue"); }
void launch_segments(const ReadDesc*, int, uint64_t, uint32_t, const ReadState*, TraceBuffers, SegRow*, int, hipStream_t, const EventCols&,
                     const KmerSummary&, const ScoreCols&, const BandMargin&) {
  no_device("launch_segments");
}
void launch_band_margin(const ReadDesc*, int, uint32_t, const ReadState*, const TraceBuffers&, const BandMargin&, hipStream_t) {
  no_device("launch_band_margin");
}
void launch_segment_scores(const ReadDesc*, int, uint64_t, uint32_t, const ReadState*, const TraceBuffers&, const ScoreCols&, hipStream_t) {
  no_device("launch_segment_scores");
}
void launch_kmer_summary(const ReadDesc*, int, uint32_t, const ReadState*, const TraceBuffers&, const KmerSummary&, hipStream_t) {
  no_device("launch_kmer_summary");
}
void launch_site_summary(const ReadDesc*, int, uint32_t, const ReadState*, const TraceBuffers&, const SiteSummary&, hipStream_t) {
  no_device("launch_site_summary");
}
void launch_site_quantiles(const SiteQuantiles&, hipStream_t) { no_device("launch_site_quantiles"); }
void launch_site_compare(const SiteCompare&, hipStream_t) { no_device("launch_site_compare"); }
void launch_site_add(const SiteAdd&, hipStream_t) { no_device("launch_site_add"); }
void launch_site_mixture(const SiteMixture&, hipStream_t) { no_device("launch_site_mixture"); }
void launch_site_gather(const SiteGather&, hipStream_t) { no_device("launch_site_gather"); }
void launch_site_scatter_add(const SiteScatter&, hipStream_t) { no_device("launch_site_scatter_add"); }
void launch_site_map_windows(const SiteWindows&, hipStream_t) { no_device("launch_site_map_windows"); }
void launch_site_pack(const SitePack&, hipStream_t) { no_device("launch_site_pack"); }
void launch_site_pack_write(const SitePack&, hipStream_t) { no_device("launch_site_pack_write"); }
void launch_site_merge(const SiteMerge&, hipStream_t) { no_device("launch_site_merge"); }
void launch_rescale_init(RescaleState*, uint64_t, hipStream_t) { no_device("launch_rescale_init"); }
void launch_rescale_pass(const ReadDesc*, int, uint32_t, const ReadState*, const TraceBuffers&, const double*, double*, const Emis*, double*,
                         RescaleState*, hipStream_t) {
  no_device("launch_rescale_pass");
}
size_t pool_stats_temp_bytes(uint64_t, uint64_t) { return 8; }
size_t pool_stats_work_bytes(uint64_t) { return 8; }
hipError_t launch_pool_stats(const ReadDesc*, int, uint32_t, const ReadState*, const int32_t*, TrainBuffers, double*, uint64_t, uint64_t, void*, void*,
                             size_t, hipStream_t) {
  no_device("launch_pool_stats");
}
uint64_t band_arena_bytes(uint64_t T, uint64_t bw, int job) { return job == 0 ? 0 : T * (2 * bw + 3) * (job == 2 ? 16 : 25); }
int band_groups_per_cu(bool, int, int) { return 1; }
hipError_t launch_band_reads(int, const BandArgs&, int, hipStream_t) { no_device("launch_band_reads"); }
void launch_guided_band_margin(const ReadDesc*, int, uint32_t, const ReadState*, const TraceBuffers&, const int32_t*, int, const BandMargin&,
                               hipStream_t, const uint8_t*) {
  no_device("launch_guided_band_margin");
}
hipError_t launch_guide_refine(const GuideRefine&, hipStream_t) { no_device("launch_guide_refine"); }
int auto_guide_groups_per_cu(int) { return 1; }
hipError_t launch_auto_guide(const AutoGuideArgs&, int, hipStream_t) { no_device("launch_auto_guide"); }
hipError_t launch_rescue_select(const RescueSelect&, hipStream_t) { no_device("launch_rescue_select"); }
hipError_t launch_rescue_merge(const RescueMerge&, hipStream_t) { no_device("launch_rescue_merge"); }

}  // namespace dynk
