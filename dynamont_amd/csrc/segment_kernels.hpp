// segment_kernels.hpp -- the per-segment kernels behind the `probability` column: the two middle order statistics of every
// segment's path posteriors pp[] (k_median: rank counting, k_median_long: radix select), their combination into the output
// row (k_final) and the three launches, text as it stood in nt_kernels.hip. Included by nt_kernels.hip (launch_segments) and
// by tests/device_math/segment_median.hip, which feeds the launches path arrays built on the host and compares every output
// bit with a sort (tests/test_gpu_segment_median.py): pp[] itself never leaves the device in the product.
// The kernels are ordinary (non-inline) definitions: one translation unit per binary includes this file.
#pragma once

#include <algorithm>

#include "nt_kernels.hpp"

namespace dynk {

// ---------------------------------------------------------------------------------------------
// K_median: formattedMedian (aligner.cpp:247-263) by rank counting. One thread per path row;
// the segment of column n spans rows [segrow[n-1], segrow[n]) (last column: up to T-1).
// Ties are broken by row so ranks are a permutation. Rank counting costs L compares per row, L^2 per
// segment: fine for the usual dwell of ~10 rows, not for a stall (a pore that sits on one k-mer for
// 20 000 samples would cost 4e8 compares); segments longer than MEDIAN_SHORT_MAX rows are left to
// k_median_long.
// ---------------------------------------------------------------------------------------------
constexpr int MEDIAN_SHORT_MAX = 256;

__global__ void k_median(const ReadDesc* __restrict__ descs, int n_reads, uint64_t rows_total, const ReadState* __restrict__ st,
                         TraceBuffers tb) {
  // one thread per path row of the WHOLE batch (rows_total = sum of T): the read is found by bisection over the
  // descriptors' path offsets (ascending in processing order). Rounds 1-3 launched max_T / 256 blocks for every read:
  // in a batch of reads of 10 k .. 100 k samples half of the blocks found nothing to do (3.8 ms per config-3 launch).
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= rows_total) return;
  int lo_i = 0, hi_i = n_reads - 1;
  while (lo_i < hi_i) {  // last read whose path_off <= g
    const int mid = (lo_i + hi_i + 1) >> 1;
    if (descs[mid].path_off <= g) lo_i = mid;
    else hi_i = mid - 1;
  }
  const ReadDesc rd = descs[lo_i];
  if (st[rd.read].status != 0) return;
  const int T = (int)rd.T, N = (int)rd.N;
  const int t = (int)(g - rd.path_off);
  if (t < 1 || t >= T) return;
  const double* __restrict__ pp = tb.pp + rd.path_off;
  const uint32_t* __restrict__ segrow = tb.segrow + rd.seg_off;
  const int n = (int)(tb.pathn[rd.path_off + t] & 0x7fffffffu);
  const int a = (int)segrow[n - 1];
  const int b = (n < N - 1) ? (int)segrow[n] : T;
  const int L = b - a;
  if (L > MEDIAN_SHORT_MAX) return;
  const double x = pp[t];
  int rank = 0;
  for (int u = a; u < b; ++u) {
    const double y = pp[u];
    rank += (y < x) || (y == x && u < t);
  }
  const int mid = L >> 1;
  if (rank == mid) tb.med_hi[rd.seg_off + n - 1] = x;
  if (!(L & 1) && rank == mid - 1) tb.med_lo[rd.seg_off + n - 1] = x;
}

// ---------------------------------------------------------------------------------------------
// K_median_long: the same two order statistics for segments longer than MEDIAN_SHORT_MAX rows, by an
// 8-bit-per-pass radix select over the bit patterns (posteriors are non-negative doubles: value order =
// unsigned order of the bits): 8 passes + 1 over the segment, O(L) instead of O(L^2). One 256-thread
// block per read; reads without a long segment leave after one strided look at their segment table.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_median_long(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                     TraceBuffers tb) {
  __shared__ uint32_t s_hist[256];
  __shared__ unsigned long long s_prefix, s_maxless;
  __shared__ uint32_t s_k, s_cntless;
  const ReadDesc rd = descs[blockIdx.x];
  if (st[rd.read].status != 0) return;
  const int T = (int)rd.T, N = (int)rd.N;
  const int tid = threadIdx.x;
  const double* __restrict__ pp = tb.pp + rd.path_off;
  const uint32_t* __restrict__ segrow = tb.segrow + rd.seg_off;
  int any = 0;
  for (int i = tid; i < N - 1; i += 256) {
    const int a = (int)segrow[i], b = (i + 1 < N - 1) ? (int)segrow[i + 1] : T;
    any |= (b - a > MEDIAN_SHORT_MAX);
  }
  if (!__syncthreads_or(any)) return;
  for (int i = 0; i < N - 1; ++i) {  // block-uniform walk over the segments of this read
    const int a = (int)segrow[i], b = (i + 1 < N - 1) ? (int)segrow[i + 1] : T;
    const int L = b - a;
    if (L <= MEDIAN_SHORT_MAX) continue;
    unsigned long long prefix = 0, mask = 0;
    uint32_t k = (uint32_t)(L >> 1);  // rank of the upper middle element
    for (int shift = 56; shift >= 0; shift -= 8) {
      s_hist[tid] = 0;
      __syncthreads();
      for (int u = a + tid; u < b; u += 256) {
        const unsigned long long bits = (unsigned long long)__double_as_longlong(pp[u]);
        if ((bits & mask) == prefix) atomicAdd(&s_hist[(bits >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (tid == 0) {
        uint32_t cum = 0, bin = 0;
        for (; bin < 255; ++bin) {
          if (k < cum + s_hist[bin]) break;
          cum += s_hist[bin];
        }
        s_k = k - cum;
        s_prefix = prefix | ((unsigned long long)bin << shift);
      }
      __syncthreads();
      prefix = s_prefix;
      k = s_k;
      mask |= 0xffull << shift;
    }
    const double hi = __longlong_as_double((long long)prefix);
    double lo = hi;
    if (!(L & 1)) {  // rank mid-1: another copy of hi, or the largest element below it
      if (tid == 0) {
        s_cntless = 0;
        s_maxless = 0;
      }
      __syncthreads();
      uint32_t cnt = 0;
      unsigned long long mx = 0;
      for (int u = a + tid; u < b; u += 256) {
        const double y = pp[u];
        if (y < hi) {
          ++cnt;
          mx = max(mx, (unsigned long long)__double_as_longlong(y));
        }
      }
      if (cnt) {
        atomicAdd(&s_cntless, cnt);
        atomicMax(&s_maxless, mx);
      }
      __syncthreads();
      if ((uint32_t)(L >> 1) - 1u < s_cntless) lo = __longlong_as_double((long long)s_maxless);
      __syncthreads();
    }
    if (tid == 0) {
      tb.med_hi[rd.seg_off + i] = hi;
      tb.med_lo[rd.seg_off + i] = lo;
    }
  }
}

// K_final: one output row per segment (NT_aligner_api.cpp:420-430).
__global__ void k_final(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                        TraceBuffers tb, SegRow* __restrict__ rows, int kmer_size) {
  const ReadDesc rd = descs[blockIdx.y];
  if (st[rd.read].status != 0) return;
  const int T = (int)rd.T, N = (int)rd.N;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;  // segment index = column - 1
  if (i >= N - 1) return;
  const uint32_t* __restrict__ segrow = tb.segrow + rd.seg_off;
  const int a = (int)segrow[i];
  const int b = (i + 1 < N - 1) ? (int)segrow[i + 1] : T;
  const int L = b - a;
  const double hi = tb.med_hi[rd.seg_off + i];
  SegRow r;
  r.signal_pos = (uint32_t)(a - 1);
  r.sequence_pos = (uint32_t)(i + kmer_size / 2);
  r.probability = (L & 1) ? hi : (tb.med_lo[rd.seg_off + i] + hi) / 2.0;
  rows[rd.seg_off + i] = r;
}

// per-read kernels put the read index in gridDim.y (<= 65 535): larger batches go in slices
constexpr int MAX_GRID_Y = 65535;

// the three launches of launch_segments (nt_kernels.hip); descs in processing order, max_N the largest ReadDesc::N
inline void launch_segment_medians(const ReadDesc* descs, int n_reads, uint64_t rows_total, uint32_t max_N, const ReadState* st,
                                   TraceBuffers tb, SegRow* rows, int kmer_size, hipStream_t s) {
  if (n_reads > 0 && rows_total)
    hipLaunchKernelGGL(k_median, dim3((unsigned)((rows_total + 255) / 256)), dim3(256), 0, s, descs, n_reads, rows_total, st, tb);
  for (int r0 = 0; r0 < n_reads; r0 += MAX_GRID_Y) {
    const int nr = std::min(MAX_GRID_Y, n_reads - r0);
    hipLaunchKernelGGL(k_median_long, dim3(nr), dim3(256), 0, s, descs + r0, st, tb);
    hipLaunchKernelGGL(k_final, dim3((max_N + 255) / 256, nr), dim3(256), 0, s, descs + r0, st, tb, rows, kmer_size);
  }
}

}  // namespace dynk
