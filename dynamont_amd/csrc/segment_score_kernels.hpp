// segment_score_kernels.hpp -- per-border segment quality scores (dyn_aligner_set_segment_scores): median_delta, mad_delta and
// homogeneity of every output row, the scores the Dynamont authors judge a segmentation by. Included by segment_scores.hip
// (launch_segment_scores) and by tests/device_math/segment_scores.hip, which feeds the launches borders built on the host and
// compares every output bit with a NumPy restatement (tests/test_gpu_segment_scores.py).
// The kernels are ordinary (non-inline) definitions: one translation unit per binary includes this file.
//
// Definition (include/dynamont_mi.h). x[0 .. S) is the signal the read queue aligned (S = T - 1,
// ReadDesc::sig_off counts from ScoreCols::sig); output row j of an ok read starts at sample p = segrow[j] - 1 and ends
// before e = segrow[j + 1] - 1 (the last one before S); W = ScoreCols::window.
//   med(v)        s[L/2] (odd L) or (s[L/2 - 1] + s[L/2]) / 2.0 (even L) of the sorted values: one IEEE add, one divide
//   mad(v)        med(|v_i - med(v)|): one IEEE subtraction and fabs per element
//   median_delta  |med(B) - med(A)|, A = x[max(0, p - W) : p], B = x[p : min(p + W, S)];  mad_delta the same with mad
//                 p == 0 (row 0): A is empty, both are NaN
//   homogeneity   L = e - p >= 10: mad(x[p + trim : e - trim]), trim = max(L / 10, 1);  otherwise NaN
// NaN is 0x7ff8000000000000. A zero of either sign may win a tie in a selection; every result ends in fabs, and neither
// fabs(a - b) nor fabs(fabs(v - m) ...) depends on the sign of a zero among its inputs, so the output bits do not either.
// Kernels:
//   k_score_window<G>  G lanes per border (G = 8 .. 64, the smallest that is >= W; a lane takes up to 4 samples), 256 / G
//                      borders per block. A half window is staged in LDS once, ranks are counted within it (ties broken by
//                      index, as k_median), the lanes of rank L/2 and L/2 - 1 deliver the median; the half is overwritten
//                      with |x - med| and counted again. A, then B. Also writes the NaN of the rows shorter than 10.
//   k_score_homog<P>   one thread per lattice row of the batch, as k_event_short: trimmed lengths up to SC_SHORT_MAX by rank
//                      counting over global memory. P = 0 leaves the trimmed median in ScoreCols::scratch, P = 1 (the next
//                      launch) counts ranks over |x - med| and writes the homogeneity.
//   k_score_long       longer trimmed segments (stalls), one 256-thread block per read: an 8-bit radix select over the
//                      order-preserving key of event_stats.hip, then again over the raw bits of |x - med| (never negative).
// No float atomics (the histograms are integer counts); no result depends on the batch around the read.
// Footprint: 256 threads; k_score_window 8.5 KB of static LDS, k_score_long 1.1 KB, k_score_homog none; no scratch memory.
#pragma once

#include <algorithm>

#include "nt_kernels.hpp"

namespace dynk {

constexpr int SC_MAX_WINDOW = 256;  // = DYN_SEGMENT_SCORES_MAX_WINDOW
constexpr int SC_SHORT_MAX = 256;   // trimmed samples: rank counting costs L^2 per segment (= EV_SHORT_MAX)
constexpr int SC_MIN_LEN = 10;      // shorter rows have no homogeneity
constexpr int SC_MAX_GRID_Y = 65535;

__device__ __forceinline__ double sc_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ double sc_median(double lo, double hi, int L) {
  return (L & 1) ? hi : __ddiv_rn(__dadd_rn(lo, hi), 2.0);
}

// The median of buf[0 .. L) (L <= 4 G; 0.0 for L == 0) for the G lanes that share buf; sel[2] is theirs too. Every thread
// of the block calls it: the barriers are the block's.
template <int G>
__device__ __forceinline__ double sc_group_median(const double* buf, int L, int lane, double* sel) {
  const int mid = L >> 1;
  for (int i = lane; i < L; i += G) {
    const double v = buf[i];
    int rank = 0;
    for (int u = 0; u < L; ++u) {
      const double y = buf[u];
      rank += (y < v) || (y == v && u < i);
    }
    if (rank == mid) sel[1] = v;
    if (rank == mid - 1) sel[0] = v;
  }
  __syncthreads();
  const double m = L > 0 ? sc_median(sel[0], sel[1], L) : 0.0;
  __syncthreads();  // sel and buf are written again after this
  return m;
}

// grid (ceil((max_N - 1) / (256 / G)), n_reads): group g of block (c, r) owns output row c * (256 / G) + g of read descs[r]
template <int G>
__global__ __launch_bounds__(256) void k_score_window(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                      const uint32_t* __restrict__ segrow_all, ScoreCols sc) {
  constexpr int NG = 256 / G;
  __shared__ double s_buf[1024];  // NG groups of W <= 4 G samples
  __shared__ double s_sel[NG][2];
  const ReadDesc rd = descs[blockIdx.y];
  const int n_seg = (int)rd.N - 1;
  if ((int)(blockIdx.x * NG) >= n_seg) return;  // (block-uniform, as the next one)
  if (st[rd.read].status != 0) return;
  const int W = min(sc.window, 4 * G);
  const int grp = (int)threadIdx.x / G, lane = (int)threadIdx.x % G;
  const int j = (int)blockIdx.x * NG + grp;
  const bool row = j < n_seg;
  const int S = (int)rd.T - 1;
  int p = 0, e = 0;
  if (row) {
    const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
    p = (int)segrow[j] - 1;
    e = (j + 1 < n_seg) ? (int)segrow[j + 1] - 1 : S;
    if (p < 0 || p >= S) p = e = 0;  // (never, for borders the traceback wrote: nothing is read out of the signal)
  }
  const double* __restrict__ x = sc.sig + rd.sig_off;
  double* buf = s_buf + grp * W;
  double* sel = s_sel[grp];
  double med[2], mad[2];
  for (int h = 0; h < 2; ++h) {
    const int lo = h == 0 ? max(0, p - W) : p;
    const int hi = h == 0 ? p : min(p + W, S);
    const int L = row ? hi - lo : 0;
    for (int i = lane; i < L; i += G) buf[i] = x[lo + i];
    __syncthreads();
    med[h] = sc_group_median<G>(buf, L, lane, sel);
    for (int i = lane; i < L; i += G) buf[i] = fabs(__dsub_rn(buf[i], med[h]));
    __syncthreads();
    mad[h] = sc_group_median<G>(buf, L, lane, sel);
  }
  if (row && lane == 0) {
    const uint64_t o = rd.seg_off + j;
    const bool has_left = p > 0;
    sc.median_delta[o] = has_left ? fabs(__dsub_rn(med[1], med[0])) : sc_nan();
    sc.mad_delta[o] = has_left ? fabs(__dsub_rn(mad[1], mad[0])) : sc_nan();
    if (e - p < SC_MIN_LEN) sc.homogeneity[o] = sc_nan();
  }
}

// one thread per lattice row of the batch (rows_total = sum of T), the read by bisection as k_median / k_event_short
template <int PHASE>
__global__ void k_score_homog(const ReadDesc* __restrict__ descs, int n_reads, uint64_t rows_total,
                              const ReadState* __restrict__ st, const uint32_t* __restrict__ pathn,
                              const uint32_t* __restrict__ segrow_all, ScoreCols sc) {
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
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  const int n = (int)(pathn[rd.path_off + t] & 0x7fffffffu);
  if (n < 1 || n > N - 1) return;
  const int a = (int)segrow[n - 1];
  const int b = (n < N - 1) ? (int)segrow[n] : T;
  const int L = b - a;
  if (L < SC_MIN_LEN || a < 1 || b > T) return;
  const int trim = max(L / 10, 1);
  const int Lt = L - 2 * trim;
  if (Lt > SC_SHORT_MAX) return;
  const int me = t - a - trim;
  if (me < 0 || me >= Lt) return;
  const double* __restrict__ xs = sc.sig + rd.sig_off + (a - 1) + trim;  // sample row - 1
  const uint64_t o = rd.seg_off + n - 1;
  const double m = PHASE ? sc.scratch[o] : 0.0;
  const double x = PHASE ? fabs(__dsub_rn(xs[me], m)) : xs[me];
  int rank = 0;
  double below = -__builtin_inf();  // the largest value ranked below x: rank Lt/2 - 1 when x has rank Lt/2
  for (int u = 0; u < Lt; ++u) {
    const double y = PHASE ? fabs(__dsub_rn(xs[u], m)) : xs[u];
    const bool less = (y < x) || (y == x && u < me);
    rank += less;
    if (less && y > below) below = y;
  }
  if (rank == (Lt >> 1)) (PHASE ? sc.homogeneity : sc.scratch)[o] = sc_median(below, x, Lt);
}

// order-preserving key of a signed double (ev_key of event_stats.hip): unsigned order of keys = value order
__device__ __forceinline__ unsigned long long sc_key(double v) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(v);
  return bits ^ ((bits >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double sc_unkey(unsigned long long k) {
  return __longlong_as_double((long long)(k ^ ((k >> 63) ? (1ull << 63) : ~0ull)));
}

struct ScSelect {  // the block's shared words of one radix select
  uint32_t hist[256];
  unsigned long long prefix, maxless;
  uint32_t k, cntless;
};

// The median of xs[0 .. L) (ABS = false) or of |xs[u] - m| (ABS = true) by the whole 256-thread block: rank L/2 by an 8-bit
// radix select over the keys, rank L/2 - 1 (even L) as another copy of it or the largest key below it.
template <bool ABS>
__device__ __forceinline__ double sc_block_median(const double* __restrict__ xs, int L, double m, ScSelect& sh) {
  const int tid = (int)threadIdx.x;
  auto key_of = [&](int u) -> unsigned long long {
    if (ABS) return (unsigned long long)__double_as_longlong(fabs(__dsub_rn(xs[u], m)));
    return sc_key(xs[u]);
  };
  unsigned long long prefix = 0, mask = 0;
  uint32_t k = (uint32_t)(L >> 1);
  for (int shift = 56; shift >= 0; shift -= 8) {
    sh.hist[tid] = 0;
    __syncthreads();
    for (int u = tid; u < L; u += 256) {
      const unsigned long long key = key_of(u);
      if ((key & mask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      uint32_t cum = 0, bin = 0;
      for (; bin < 255; ++bin) {
        if (k < cum + sh.hist[bin]) break;
        cum += sh.hist[bin];
      }
      sh.k = k - cum;
      sh.prefix = prefix | ((unsigned long long)bin << shift);
    }
    __syncthreads();
    prefix = sh.prefix;
    k = sh.k;
    mask |= 0xffull << shift;
  }
  unsigned long long lo_key = prefix;
  if (!(L & 1)) {
    if (tid == 0) {
      sh.cntless = 0;
      sh.maxless = 0;
    }
    __syncthreads();
    uint32_t cnt = 0;
    unsigned long long mx = 0;
    for (int u = tid; u < L; u += 256) {
      const unsigned long long key = key_of(u);
      if (key < prefix) {
        ++cnt;
        mx = max(mx, key);
      }
    }
    if (cnt) {
      atomicAdd(&sh.cntless, cnt);
      atomicMax(&sh.maxless, mx);
    }
    __syncthreads();
    if ((uint32_t)(L >> 1) - 1u < sh.cntless) lo_key = sh.maxless;
    __syncthreads();
  }
  const double hi = ABS ? __longlong_as_double((long long)prefix) : sc_unkey(prefix);
  const double lo = ABS ? __longlong_as_double((long long)lo_key) : sc_unkey(lo_key);
  return sc_median(lo, hi, L);
}

__device__ __forceinline__ int sc_trimmed(int L) { return L < SC_MIN_LEN ? 0 : L - 2 * max(L / 10, 1); }

__global__ __launch_bounds__(256) void k_score_long(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                    const uint32_t* __restrict__ segrow_all, ScoreCols sc) {
  __shared__ ScSelect sh;
  const ReadDesc rd = descs[blockIdx.x];
  if (st[rd.read].status != 0) return;
  const int T = (int)rd.T, n_seg = (int)rd.N - 1;
  const int tid = (int)threadIdx.x;
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  int any = 0;
  for (int i = tid; i < n_seg; i += 256) {
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    any |= (sc_trimmed(b - a) > SC_SHORT_MAX);
  }
  if (!__syncthreads_or(any)) return;
  for (int i = 0; i < n_seg; ++i) {  // block-uniform walk over the segments of this read
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    const int L = b - a;
    const int Lt = sc_trimmed(L);
    if (Lt <= SC_SHORT_MAX || a < 1 || b > T) continue;
    const double* __restrict__ xs = sc.sig + rd.sig_off + (a - 1) + max(L / 10, 1);
    const double m = sc_block_median<false>(xs, Lt, 0.0, sh);
    const double h = sc_block_median<true>(xs, Lt, m, sh);
    if (tid == 0) sc.homogeneity[rd.seg_off + i] = h;
  }
}

template <int G>
inline void launch_score_window(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const uint32_t* segrow,
                                const ScoreCols& sc, hipStream_t s) {
  constexpr unsigned NG = 256 / G;
  for (int r0 = 0; r0 < n_reads; r0 += SC_MAX_GRID_Y) {
    const int nr = std::min(SC_MAX_GRID_Y, n_reads - r0);
    hipLaunchKernelGGL(k_score_window<G>, dim3((max_N - 1 + NG - 1) / NG, (unsigned)nr), dim3(256), 0, s, descs + r0, st, segrow, sc);
  }
}

// the launches of launch_segment_scores (segment_scores.hip); descs in processing order, max_N the largest ReadDesc::N.
// The columns were zeroed by the caller: rows of failed reads keep the zeros.
inline void launch_segment_score_kernels(const ReadDesc* descs, int n_reads, uint64_t rows_total, uint32_t max_N,
                                         const ReadState* st, const uint32_t* pathn, const uint32_t* segrow, const ScoreCols& sc,
                                         hipStream_t s) {
  if (!sc.median_delta || sc.window < 1 || sc.window > SC_MAX_WINDOW || n_reads <= 0 || max_N < 2 || !rows_total) return;
  if (sc.window <= 8) launch_score_window<8>(descs, n_reads, max_N, st, segrow, sc, s);
  else if (sc.window <= 16) launch_score_window<16>(descs, n_reads, max_N, st, segrow, sc, s);
  else if (sc.window <= 32) launch_score_window<32>(descs, n_reads, max_N, st, segrow, sc, s);
  else launch_score_window<64>(descs, n_reads, max_N, st, segrow, sc, s);
  const dim3 per_row((unsigned)((rows_total + 255) / 256));
  hipLaunchKernelGGL(k_score_homog<0>, per_row, dim3(256), 0, s, descs, n_reads, rows_total, st, pathn, segrow, sc);
  hipLaunchKernelGGL(k_score_homog<1>, per_row, dim3(256), 0, s, descs, n_reads, rows_total, st, pathn, segrow, sc);
  hipLaunchKernelGGL(k_score_long, dim3((unsigned)n_reads), dim3(256), 0, s, descs, st, segrow, sc);
}

}  // namespace dynk
