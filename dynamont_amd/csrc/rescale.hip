// rescale.hip -- per-read signal rescaling (dyn_aligner_set_rescale): between two passes of align(calc_probabilities = 1),
// a least-squares fit of each read's segment levels on the model levels of the k-mers that scored them updates the read's
// affine transform, and its signal is recomputed from the kept preprocessed signal x0. Definition, bit for bit
// (include/dynamont_mi.h, INTEGRATION.md section 3, tests/rescale_chain.py):
//   y_j   level_mean of output row j over x_k (ABI 9: chunks of 64 samples, each left to right, the chunk sums left to right)
//   m_j   model level_mean of the k-mer of lattice column j + 1 (the row's motif): ReadDesc::par_off + j
//   S     a sum over the n rows in chunks of 64 consecutive rows, each chunk left to right, the chunk sums left to right
//   mbar = S(m) / n, ybar = S(y) / n, Sxx = S((m - mbar)^2), Sxy = S((m - mbar) * (y - ybar)), b = Sxy / Sxx,
//   a = ybar - b * mbar -- one IEEE fp64 operation each, no contraction
//   applied when n >= 16, Sxx > 0, a and b finite, 0.5 <= b <= 2, |a| <= 2: A += B * a, B *= b; else the read's later fits
//   are skipped too (as are those of a read that failed)
//   x_{k+1}[i] = (x0[i] - A) / B
// Three kernels: k_rescale_init (A = 0, B = 1 for every read of the batch), k_rescale_fit (one 256-thread workgroup per read:
// the row means into a scratch column -- one lane per short segment, all lanes over the chunks of a stall, as k_event_long --
// then the four chunked row sums, chunk c by lane c mod 256 and the chunk sums in order by lane 0), k_rescale_apply (one
// workgroup per fitted read over its samples). No atomics: results are identical run to run.
#include "nt_kernels.hpp"

#include <algorithm>

namespace dynk {

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_CHUNK = 64;        // samples per chunk of a segment mean, rows per chunk of the fit's sums
constexpr int RS_SHORT_MAX = 256;   // segments up to this length: one lane each; longer ones: the whole workgroup
constexpr int RS_MIN_ROWS = 16;
constexpr int RS_GRID_Y = 65535;

__device__ __forceinline__ double rs_chunked_sum(const double* __restrict__ x, int L) {
  double s = 0.0;
  for (int c0 = 0; c0 < L; c0 += RS_CHUNK) {
    const int c1 = min(c0 + RS_CHUNK, L);
    double cs = x[c0];
    for (int j = c0 + 1; j < c1; ++j) cs = __dadd_rn(cs, x[j]);
    s = c0 == 0 ? cs : __dadd_rn(s, cs);
  }
  return s;
}

// S over rows 0 .. n-1 of term(j), by the whole workgroup; the result in every lane. s_part: RS_THREADS doubles of LDS.
template <class F>
__device__ __forceinline__ double rs_row_sum(int n, F term, double* s_part, double* s_out) {
  const int tid = threadIdx.x;
  const int n_chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
  double acc = 0.0;
  for (int c0 = 0; c0 < n_chunks; c0 += RS_THREADS) {
    const int c = c0 + tid;
    if (c < n_chunks) {
      const int j0 = c * RS_CHUNK, j1 = min(j0 + RS_CHUNK, n);
      double cs = term(j0);
      for (int j = j0 + 1; j < j1; ++j) cs = __dadd_rn(cs, term(j));
      s_part[tid] = cs;
    }
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < min(RS_THREADS, n_chunks - c0); ++j) acc = (c0 + j == 0) ? s_part[j] : __dadd_rn(acc, s_part[j]);
    __syncthreads();
  }
  if (tid == 0) *s_out = acc;
  __syncthreads();
  const double r = *s_out;
  __syncthreads();
  return r;
}

__global__ void k_rescale_init(RescaleState* __restrict__ rs, uint64_t n_reads) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_reads) return;
  RescaleState s{};
  s.A = 0.0;
  s.B = 1.0;
  rs[i] = s;
}

__global__ __launch_bounds__(RS_THREADS) void k_rescale_fit(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                            const uint32_t* __restrict__ segrow_all, const double* __restrict__ sig,
                                                            const Emis* __restrict__ par, double* __restrict__ y_all,
                                                            RescaleState* __restrict__ rs) {
  __shared__ double s_part[RS_THREADS];
  __shared__ double s_val;
  const ReadDesc rd = descs[blockIdx.x];
  const int tid = threadIdx.x;
  RescaleState* __restrict__ me = rs + rd.read;
  const bool failed = st[rd.read].status != 0;
  if (failed || me->frozen) {
    __syncthreads();  // every lane has read `frozen` before it is written
    if (tid == 0) {
      me->fitted = 0;
      me->frozen = 1;
    }
    return;
  }
  const int T = (int)rd.T, n = (int)rd.N - 1;
  if (n < RS_MIN_ROWS) {
    __syncthreads();
    if (tid == 0) {
      me->fitted = 0;
      me->frozen = 1;
    }
    return;
  }
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  const double* __restrict__ x = sig + rd.sig_off;
  double* __restrict__ y = y_all + rd.seg_off;
  // ---- the row means: short segments one lane each, stalls by the whole workgroup ----
  int any_long = 0;
  for (int j = tid; j < n; j += RS_THREADS) {
    const int a = (int)segrow[j], b = (j + 1 < n) ? (int)segrow[j + 1] : T;
    const int L = b - a;
    if (L > RS_SHORT_MAX) any_long = 1;
    else y[j] = __ddiv_rn(rs_chunked_sum(x + (a - 1), L), (double)L);  // sample row - 1
  }
  if (__syncthreads_or(any_long)) {
    for (int j = 0; j < n; ++j) {  // workgroup-uniform walk
      const int a = (int)segrow[j], b = (j + 1 < n) ? (int)segrow[j + 1] : T;
      const int L = b - a;
      if (L <= RS_SHORT_MAX) continue;
      const double* __restrict__ xs = x + (a - 1);
      const int n_chunks = (L + RS_CHUNK - 1) / RS_CHUNK;
      double acc = 0.0;
      for (int c0 = 0; c0 < n_chunks; c0 += RS_THREADS) {
        const int c = c0 + tid;
        if (c < n_chunks) s_part[tid] = rs_chunked_sum(xs + c * RS_CHUNK, min(RS_CHUNK, L - c * RS_CHUNK));
        __syncthreads();
        if (tid == 0)
          for (int u = 0; u < min(RS_THREADS, n_chunks - c0); ++u) acc = (c0 + u == 0) ? s_part[u] : __dadd_rn(acc, s_part[u]);
        __syncthreads();
      }
      if (tid == 0) y[j] = __ddiv_rn(acc, (double)L);
    }
  }
  __syncthreads();  // the row means are visible to the whole workgroup
  // ---- the fit ----
  const Emis* __restrict__ pm = par + rd.par_off;  // row j <-> column j + 1 <-> entry j
  const double dn = (double)n;
  const double mbar = __ddiv_rn(rs_row_sum(n, [&](int j) { return pm[j].mean; }, s_part, &s_val), dn);
  const double ybar = __ddiv_rn(rs_row_sum(n, [&](int j) { return y[j]; }, s_part, &s_val), dn);
  const double sxx = rs_row_sum(
      n, [&](int j) { const double d = __dsub_rn(pm[j].mean, mbar); return __dmul_rn(d, d); }, s_part, &s_val);
  const double sxy = rs_row_sum(
      n, [&](int j) { return __dmul_rn(__dsub_rn(pm[j].mean, mbar), __dsub_rn(y[j], ybar)); }, s_part, &s_val);
  if (tid == 0) {
    const double b = __ddiv_rn(sxy, sxx);
    const double a = __dsub_rn(ybar, __dmul_rn(b, mbar));
    const bool ok = sxx > 0.0 && isfinite(a) && isfinite(b) && b >= 0.5 && b <= 2.0 && fabs(a) <= 2.0;
    if (ok) {
      const double A = me->A, B = me->B;
      me->A = __dadd_rn(A, __dmul_rn(B, a));
      me->B = __dmul_rn(B, b);
      me->applied += 1;
      me->fitted = 1;
    } else {
      me->fitted = 0;
      me->frozen = 1;
    }
  }
}

__global__ void k_rescale_apply(const ReadDesc* __restrict__ descs, const RescaleState* __restrict__ rs,
                                const double* __restrict__ sig0, double* __restrict__ sig) {
  const ReadDesc rd = descs[blockIdx.y];
  const RescaleState s = rs[rd.read];
  if (!s.fitted) return;
  const uint64_t S = (uint64_t)rd.T - 1;
  const double* __restrict__ x0 = sig0 + rd.sig_off;
  double* __restrict__ x = sig + rd.sig_off;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (uint64_t)gridDim.x * blockDim.x)
    x[i] = __ddiv_rn(__dsub_rn(x0[i], s.A), s.B);
}

}  // namespace

void launch_rescale_init(RescaleState* rs, uint64_t n_reads, hipStream_t s) {
  if (!n_reads) return;
  hipLaunchKernelGGL(k_rescale_init, dim3((unsigned)((n_reads + 255) / 256)), dim3(256), 0, s, rs, n_reads);
}

void launch_rescale_pass(const ReadDesc* descs, int n_reads, uint32_t max_T, const ReadState* st, const TraceBuffers& tb,
                         const double* sig0, double* sig, const Emis* par, double* y, RescaleState* rs, hipStream_t s) {
  if (n_reads <= 0) return;
  hipLaunchKernelGGL(k_rescale_fit, dim3((unsigned)n_reads), dim3(RS_THREADS), 0, s, descs, st, tb.segrow, sig, par, y, rs);
  // samples over x (up to 16 workgroups of 256 per read), reads over y
  const unsigned gx = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(16, ((uint64_t)max_T + 255) / 256));
  for (int r0 = 0; r0 < n_reads; r0 += RS_GRID_Y) {
    const int nr = std::min(RS_GRID_Y, n_reads - r0);
    hipLaunchKernelGGL(k_rescale_apply, dim3(gx, (unsigned)nr), dim3(256), 0, s, descs + r0, rs, sig0, sig);
  }
}

}  // namespace dynk
