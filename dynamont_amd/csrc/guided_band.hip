// guided_band.hip -- what a guided batch (dyn_batch_set_guide) runs beside the banded-lattice kernel (band_reads.hip, GuideWindow):
// its band margins, taken against the guide's window, and the guide refinement (dyn_batch_set_guide_refine).
#include "guided_band_kernels.hpp"

namespace dynk {

namespace {
constexpr uint32_t GBM_NONE = 0xffffffffu;  // DYN_BAND_MARGIN_NONE
}

// ---- guided band margins: one thread per path row ----
// grid ceil((read_hi - read_lo) / 256)
// only: a per-read code (the guide rescue's); the reads whose code is 1 alone are initialised and computed. Null: every read
__global__ __launch_bounds__(256) void k_bmargin_guided_init(BandMargin bm, const uint8_t* __restrict__ only) {
  const uint64_t i = (uint64_t)bm.read_lo + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= bm.read_hi) return;
  if (only && only[i] != 1) return;
  bm.low[i] = GBM_NONE;
  bm.high[i] = GBM_NONE;
  bm.edge_rows[i] = 0u;
}

// grid (n_reads, ceil(max_T / 256)): thread j of block (r, c) owns lattice row c * 256 + j of read descs[r]
__global__ __launch_bounds__(256) void k_bmargin_guided(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                        const uint32_t* __restrict__ pathn_all, const uint32_t* __restrict__ segrow_all,
                                                        const int32_t* __restrict__ guide, int bw, BandMargin bm,
                                                        const uint8_t* __restrict__ only) {
  const ReadDesc rd = descs[blockIdx.x];
  const int T = (int)rd.T, N = (int)rd.N;
  if ((int)(blockIdx.y * 256u) >= T || N < 2) return;
  if (only && only[rd.read] != 1) return;
  if (rd.read < bm.read_lo || rd.read >= bm.read_hi || st[rd.read].status != 0) return;
  const int t = (int)(blockIdx.y * 256u + threadIdx.x);
  uint32_t low = GBM_NONE, high = GBM_NONE, edge = 0u;
  if (t < T && t >= 1 && t >= (int)segrow_all[rd.seg_off]) {
    const int n = (int)(pathn_all[rd.path_off + t] & 0x7fffffffu);
    const int mid = (int)guide[rd.sig_off + t - 1];
    bool zero = false;
    if (mid - bw >= 2) {  // the lower edge is real: a column of 1 .. N-1 below the window is excluded
      low = (uint32_t)(n - (mid - bw));
      zero |= low == 0u;
    }
    if (mid + bw + 1 < N) {  // the upper edge is real
      high = (uint32_t)((mid + bw) - n);
      zero |= high == 0u;
    }
    edge = zero ? 1u : 0u;  // a row where both slacks are 0 counts once
  }
  for (int d = warpSize >> 1; d > 0; d >>= 1) {
    low = min(low, (uint32_t)__shfl_down(low, d));
    high = min(high, (uint32_t)__shfl_down(high, d));
    edge += (uint32_t)__shfl_down(edge, d);
  }
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (low != GBM_NONE) atomicMin(bm.low + rd.read, low);
    if (high != GBM_NONE) atomicMin(bm.high + rd.read, high);
    if (edge) atomicAdd(bm.edge_rows + rd.read, edge);
  }
}

void launch_guided_band_margin(const ReadDesc* descs, int n_reads, uint32_t max_T, const ReadState* st, const TraceBuffers& tb,
                               const int32_t* guide, int bw, const BandMargin& bm, hipStream_t s, const uint8_t* only) {
  if (!bm.low || bm.read_lo >= bm.read_hi) return;
  hipLaunchKernelGGL(k_bmargin_guided_init, dim3((bm.read_hi - bm.read_lo + 255u) / 256u), dim3(256), 0, s, bm, only);
  if (n_reads <= 0 || max_T < 2) return;
  hipLaunchKernelGGL(k_bmargin_guided, dim3((unsigned)n_reads, (max_T + 255u) / 256u), dim3(256), 0, s, descs, st, tb.pathn,
                     tb.segrow, guide, bw, bm, only);
}

// ---- guide refinement (dyn_batch_set_guide_refine): the called path becomes the next guide ----
// grid n_reads x 256 threads: block k owns entry k of the list of reads the launch before it aligned (active_in; null: every
// descriptor). The read's alignment is counted; an ok read's next guide g'[s] = pathn[s + 1] (0 before the first border) is
// compared with its guide. Equal in every entry: the read has converged, its result stands. Otherwise, unless this was the last
// round, g' replaces the guide and the read joins active_out, the list of the next launch.
__global__ __launch_bounds__(256) void k_guide_refine(const GuideRefine r) {
  const uint32_t n_in = r.active_in ? *r.n_in : (uint32_t)r.n_reads;
  if (blockIdx.x >= n_in) return;
  const uint32_t idx = r.active_in ? r.active_in[blockIdx.x] : blockIdx.x;
  if (idx >= (uint32_t)r.n_reads) return;
  const ReadDesc rd = r.descs[idx];
  if (threadIdx.x == 0) r.rounds[rd.read] += 1u;
  if (r.st[rd.read].status != 0) return;  // (the read's last alignment failed: that is its result)
  const int T = (int)rd.T;
  const int first = rd.N >= 2 ? (int)r.segrow[rd.seg_off] : T;  // lattice row of the first border
  const uint32_t* __restrict__ pathn = r.pathn + rd.path_off;
  int32_t* gd = r.guide + rd.sig_off;
  int differs = 0;
  for (int s = (int)threadIdx.x; s < T - 1; s += 256) {
    const int32_t g = s + 1 >= first ? (int32_t)(pathn[s + 1] & 0x7fffffffu) : 0;
    differs |= g != gd[s];
  }
  if (!__syncthreads_or(differs)) {
    if (threadIdx.x == 0) r.converged[rd.read] = 1u;
    return;
  }
  if (r.last) return;
  for (int s = (int)threadIdx.x; s < T - 1; s += 256) gd[s] = s + 1 >= first ? (int32_t)(pathn[s + 1] & 0x7fffffffu) : 0;
  if (threadIdx.x == 0) r.active_out[atomicAdd(r.n_out, 1u)] = idx;
}

hipError_t launch_guide_refine(const GuideRefine& r, hipStream_t s) {
  if (r.n_reads <= 0) return hipSuccess;
  if (!r.rounds || !r.converged || !r.guide || !r.active_out || !r.n_out || (r.active_in && !r.n_in)) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(r.n_out, 0, 4, s)) return e;
  hipLaunchKernelGGL(k_guide_refine, dim3((unsigned)r.n_reads), dim3(256), 0, s, r);
  return hipGetLastError();
}

}  // namespace dynk
