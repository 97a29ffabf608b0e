// event_stats.hip -- per-segment signal levels (dyn_aligner_set_event_stats): level_mean, level_stdv, level_median of the
// aligned signal over each output row's samples, the per-event columns of f5c eventalign / Uncalled4.
//
// Segment i of a read covers lattice rows [segrow[i], segrow[i+1]) (the last one up to T), i.e. samples row - 1 of the
// signal the read queue aligned (ReadDesc::sig_off counts from the pointer passed here). Definition, bit for bit
// (tests/test_event_stats_host.py):
//   sums        chunks of 64 consecutive samples from the segment's first; each chunk summed left to right from its first
//               element, the chunk sums left to right from the first -- one IEEE fp64 operation each, no contraction
//   level_mean  S / L                         level_stdv  sqrt(Q / L), Q the same chunked sum of (x - mean)^2
//   level_median  s[L/2] (odd L) or (s[L/2 - 1] + s[L/2]) / 2 (even L), then + 0.0 (no -0.000000 in the CSV)
// Two kernels, split like k_median / k_median_long:
//   k_event_short  one thread per lattice row of the batch; the thread of a segment's first row sums it (one lane per
//                  segment), every thread counts its sample's rank (ties broken by row, as k_median) and the thread of
//                  rank L/2 writes the median -- it has the largest sample below it (rank L/2 - 1) from the same loop
//   k_event_long   segments longer than EV_SHORT_MAX rows, one 256-thread block per read: lanes sum chunks in parallel,
//                  one lane combines the chunk sums in order; the median by an 8-bit radix select over an order-preserving
//                  key of the signed doubles. (k_median_long's select works on raw bits -- its posteriors are never
//                  negative -- and is left as it is; it is pinned bit for bit by tests/test_gpu_segment_median.py.)
// No float atomics (the histograms are integer counts): results are identical run to run.
#include "nt_kernels.hpp"

namespace dynk {

namespace {

constexpr int EV_SHORT_MAX = 256;  // = MEDIAN_SHORT_MAX: rank counting costs L^2 per segment
constexpr int EV_CHUNK = 64;

// the chunked sum of the definition over x[0 .. L)
__device__ __forceinline__ double chunked_sum(const double* __restrict__ x, int L) {
  double s = 0.0;
  for (int c0 = 0; c0 < L; c0 += EV_CHUNK) {
    const int c1 = min(c0 + EV_CHUNK, L);
    double cs = x[c0];
    for (int j = c0 + 1; j < c1; ++j) cs = __dadd_rn(cs, x[j]);
    s = c0 == 0 ? cs : __dadd_rn(s, cs);
  }
  return s;
}

__device__ __forceinline__ double chunked_sq_dev(const double* __restrict__ x, int L, double mean) {
  double s = 0.0;
  for (int c0 = 0; c0 < L; c0 += EV_CHUNK) {
    const int c1 = min(c0 + EV_CHUNK, L);
    double d = __dsub_rn(x[c0], mean);
    double cs = __dmul_rn(d, d);
    for (int j = c0 + 1; j < c1; ++j) {
      d = __dsub_rn(x[j], mean);
      cs = __dadd_rn(cs, __dmul_rn(d, d));
    }
    s = c0 == 0 ? cs : __dadd_rn(s, cs);
  }
  return s;
}

// order-preserving key of a signed double: unsigned order of keys = value order (-0.0 sorts just below +0.0)
__device__ __forceinline__ uint64_t ev_key(double v) {
  const uint64_t bits = (uint64_t)__double_as_longlong(v);
  return bits ^ ((bits >> 63) ? ~0ull : (1ull << 63));
}
__device__ __forceinline__ double ev_unkey(uint64_t k) {
  return __longlong_as_double((long long)(k ^ ((k >> 63) ? (1ull << 63) : ~0ull)));
}

__device__ __forceinline__ double ev_median(double lo, double hi, int L) {
  const double m = (L & 1) ? hi : __ddiv_rn(__dadd_rn(lo, hi), 2.0);
  return __dadd_rn(m, 0.0);
}

__global__ void k_event_short(const ReadDesc* __restrict__ descs, int n_reads, uint64_t rows_total,
                              const ReadState* __restrict__ st, const uint32_t* __restrict__ pathn,
                              const uint32_t* __restrict__ segrow_all, const double* __restrict__ sig, EventCols ev) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= rows_total) return;
  int lo_i = 0, hi_i = n_reads - 1;
  while (lo_i < hi_i) {  // last read whose path_off <= g (as k_median)
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
  const int a = (int)segrow[n - 1];
  const int b = (n < N - 1) ? (int)segrow[n] : T;
  const int L = b - a;
  if (L > EV_SHORT_MAX) return;
  const double* __restrict__ xs = sig + rd.sig_off + (a - 1);  // sample row - 1
  const uint64_t o = rd.seg_off + n - 1;
  if (t == a) {
    const double mean = __ddiv_rn(chunked_sum(xs, L), (double)L);
    ev.mean[o] = mean;
    ev.stdev[o] = __dsqrt_rn(__ddiv_rn(chunked_sq_dev(xs, L, mean), (double)L));
  }
  const int me = t - a;
  const double x = xs[me];
  int rank = 0;
  double below = -__builtin_inf();  // the largest sample ranked below x: rank L/2 - 1 when x has rank L/2
  for (int u = 0; u < L; ++u) {
    const double y = xs[u];
    const bool less = (y < x) || (y == x && u < me);
    rank += less;
    if (less && y > below) below = y;
  }
  if (rank == (L >> 1)) ev.median[o] = ev_median(below, x, L);
}

__global__ __launch_bounds__(256) void k_event_long(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                    const uint32_t* __restrict__ segrow_all, const double* __restrict__ sig,
                                                    EventCols ev) {
  __shared__ double s_part[256];
  __shared__ double s_mean;
  __shared__ uint32_t s_hist[256];
  __shared__ unsigned long long s_prefix, s_maxless;
  __shared__ uint32_t s_k, s_cntless;
  const ReadDesc rd = descs[blockIdx.x];
  if (st[rd.read].status != 0) return;
  const int T = (int)rd.T, N = (int)rd.N;
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  int any = 0;
  for (int i = tid; i < N - 1; i += 256) {
    const int a = (int)segrow[i], b = (i + 1 < N - 1) ? (int)segrow[i + 1] : T;
    any |= (b - a > EV_SHORT_MAX);
  }
  if (!__syncthreads_or(any)) return;
  for (int i = 0; i < N - 1; ++i) {  // block-uniform walk over the segments of this read
    const int a = (int)segrow[i], b = (i + 1 < N - 1) ? (int)segrow[i + 1] : T;
    const int L = b - a;
    if (L <= EV_SHORT_MAX) continue;
    const double* __restrict__ xs = sig + rd.sig_off + (a - 1);
    const int n_chunks = (L + EV_CHUNK - 1) / EV_CHUNK;
    // ---- sums: chunk c by lane c mod 256, the chunk sums in order by lane 0 ----
    double acc = 0.0;  // lane 0's running total
    for (int c0 = 0; c0 < n_chunks; c0 += 256) {
      const int c = c0 + tid;
      if (c < n_chunks) s_part[tid] = chunked_sum(xs + c * EV_CHUNK, min(EV_CHUNK, L - c * EV_CHUNK));
      __syncthreads();
      if (tid == 0)
        for (int j = 0; j < min(256, n_chunks - c0); ++j) acc = (c0 + j == 0) ? s_part[j] : __dadd_rn(acc, s_part[j]);
      __syncthreads();
    }
    if (tid == 0) s_mean = __ddiv_rn(acc, (double)L);
    __syncthreads();
    const double mean = s_mean;
    for (int c0 = 0; c0 < n_chunks; c0 += 256) {
      const int c = c0 + tid;
      if (c < n_chunks) s_part[tid] = chunked_sq_dev(xs + c * EV_CHUNK, min(EV_CHUNK, L - c * EV_CHUNK), mean);
      __syncthreads();
      if (tid == 0)
        for (int j = 0; j < min(256, n_chunks - c0); ++j) acc = (c0 + j == 0) ? s_part[j] : __dadd_rn(acc, s_part[j]);
      __syncthreads();
    }
    // ---- median: radix select of rank L/2 over the keys, 8 bits per pass ----
    unsigned long long prefix = 0, mask = 0;
    uint32_t k = (uint32_t)(L >> 1);
    for (int shift = 56; shift >= 0; shift -= 8) {
      s_hist[tid] = 0;
      __syncthreads();
      for (int u = tid; u < L; u += 256) {
        const unsigned long long key = ev_key(xs[u]);
        if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
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
    unsigned long long lo_key = prefix;
    if (!(L & 1)) {  // rank L/2 - 1: another copy of the upper element, or the largest key below it
      if (tid == 0) {
        s_cntless = 0;
        s_maxless = 0;
      }
      __syncthreads();
      uint32_t cnt = 0;
      unsigned long long mx = 0;
      for (int u = tid; u < L; u += 256) {
        const unsigned long long key = ev_key(xs[u]);
        if (key < prefix) {
          ++cnt;
          mx = max(mx, key);
        }
      }
      if (cnt) {
        atomicAdd(&s_cntless, cnt);
        atomicMax(&s_maxless, mx);
      }
      __syncthreads();
      if ((uint32_t)(L >> 1) - 1u < s_cntless) lo_key = s_maxless;
      __syncthreads();
    }
    if (tid == 0) {
      const uint64_t o = rd.seg_off + i;
      ev.mean[o] = mean;
      ev.stdev[o] = __dsqrt_rn(__ddiv_rn(acc, (double)L));
      ev.median[o] = ev_median(ev_unkey(lo_key), ev_unkey(prefix), L);
    }
  }
}

}  // namespace

void launch_event_stats(const ReadDesc* descs, int n_reads, uint64_t rows_total, const ReadState* st, const TraceBuffers& tb,
                        const EventCols& ev, hipStream_t s) {
  if (!ev.mean || n_reads <= 0 || !rows_total) return;
  hipLaunchKernelGGL(k_event_short, dim3((unsigned)((rows_total + 255) / 256)), dim3(256), 0, s, descs, n_reads, rows_total, st,
                     tb.pathn, tb.segrow, ev.sig, ev);
  hipLaunchKernelGGL(k_event_long, dim3((unsigned)n_reads), dim3(256), 0, s, descs, st, tb.segrow, ev.sig, ev);
}

}  // namespace dynk
