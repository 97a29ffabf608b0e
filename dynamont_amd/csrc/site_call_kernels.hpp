// site_call_kernels.hpp -- per-read site calls (dyn_aligner_set_site_calls): every output row of an align(calc = 1) job scored
// against the per-site model the caller uploaded (dyn_aligner_set_site_model), as a z-score under component 0 and as the
// posterior probability of component 1 of the site's two-component mixture. Included by site_summary.hip (launch_site_calls,
// launch_site_model_scatter, launch_site_model_gather) and by tests/device_math/site_calls.hip, which runs the kernels on arrays the
// test uploads and compares every double by its bits with a restatement in Python floats (tests/site_call_cases.py,
// tests/test_gpu_site_calls.py). The kernels are ordinary (non-inline) definitions: one translation unit per binary includes this file.
//
// Definition. The model: one row of five doubles pi1, mu0, mu1, var0, var1 per table row (dense: per
// site id; sparse: per bucket of the map), zeroed at allocation.
//   set            var0 > 0 and mu0, var0 finite
//   two-component  set, 0 < pi1 < 1, var1 > 0 and mu1, var1 finite
// Output row j of an ok read: id s = sites[par_off + j], L samples, m = __ddiv_rn(S1, (double)L) with S1 the chunked sum of the site
// summary (xs_chunked_sum; rows above SS_SHORT_MAX samples: the chunk sums added in order by one lane) -- level_mean of
// dyn_event_out bit for bit.
//   no call   both outputs the NaN 0x7FF8000000000000: no ids staged, no model uploaded, s == DYN_SITE_NONE, s >= num_sites, L or
//             the row's borders outside the kernels' bounds, m non-finite or m * m >= 2^64, no bucket for s in a sparse map, the
//             model row not set
//   site_z            __ddiv_rn(__dadd_rn(m, -mu0), __dsqrt_rn(var0))
//   site_probability  the NaN unless the row is two-component; then pi0 = __dadd_rn(1.0, -pi1) and g_1 of the mixture's E-step
//                     (sm_estep<1>, site_mixture_kernels.hpp) at x = m: A_k = pi_k / sqrt(var_k), d_k = m - mu_k,
//                     q_k = -0.5 * ((d_k * d_k) / var_k), up = q_1 > q_0, ONE exp_strict of the smaller q minus the larger, the
//                     other factor 1.0, p_k = A_k * factor_k, s = p_0 + p_1, p_1 / s. A quotient that is no number is written as
//                     the NaN above.
// No logarithm, no float atomics, no shuffles. The call kernels only FIND a bucket (sm_find): they never insert a key.
//
// Two kernels, split like k_ssum_short / k_ssum_long at SS_SHORT_MAX samples, the same summation order:
//   k_scall_short  one thread per OUTPUT row: block (read, chunk of 256 rows); also writes the NaN of the rows whose borders are
//                  out of bounds
//   k_scall_long   one 256-thread block per read that has a longer row: lanes sum chunks in parallel, lane 0 adds the chunk sums
//                  in order (the chunk loop wraps beyond 256 chunks) and scores the row
// Every output row of every ok read in [read_lo, read_hi) is written exactly once; rows of other reads are left alone.
// Footprint: 256 threads, 2 KB (short) / 4.25 KB (long: the chunk sums and the block-wide vote on top) of static LDS -- the strict
// exp table, staged once per block from the engine's device copy: the lookup is lane-divergent --, 26 / 42 VGPRs, no scratch: they
// run beside a resident workgroup (profiles/site_calls/kernel_text.txt).
//
// The model's window calls: k_site_model_scatter writes a staged window of rows into the rows of its ids of a SPARSE table (a set
// row finds or inserts its bucket, as k_site_scatter_add does; a row that is not set inserts nothing and clears the bucket its id
// already has; a set row without a bucket is counted), k_site_model_gather reads a window of ids back (an absent id: zeros).
#pragma once

#include "exact_sum_kernels.hpp"
#include "nt_kernels.hpp"
#include "site_map.hpp"
#include "site_mixture_kernels.hpp"
#include "site_summary_kernels.hpp"

namespace dynk {

__device__ __forceinline__ double sc_nan() { return __longlong_as_double(0x7FF8000000000000ll); }
__device__ __forceinline__ bool sc_finite(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7FF0000000000000ull) != 0x7FF0000000000000ull; }
__device__ __forceinline__ bool sc_row_set(double mu0, double var0) { return var0 > 0.0 && sc_finite(mu0) && sc_finite(var0); }

// one row with a usable id (id < num_sites, a model, L inside the bounds): prob and z as the definition gives them
__device__ __forceinline__ void sc_evaluate(const SiteCalls& sc, uint32_t id, int L, double s1, const uint64_t* tab, double& prob, double& z) {
  prob = sc_nan();
  z = sc_nan();
  const double m = __ddiv_rn(s1, (double)L);
  const double mm = __dmul_rn(m, m);
  if (!(mm < XS_TWO64)) return;  // NaN and +-inf fail the comparison too
  uint32_t row = id;
  if (sc.map_keys) {  // sparse: found or no call -- never inserted
    row = sm_find(sc.map_keys, sc.capacity, id);
    if (row == SM_NO_ROW) return;
  }
  const double* __restrict__ p = sc.model + (uint64_t)row * SC_MODEL_FIELDS;
  const double pi1 = p[0], mu0 = p[1], mu1 = p[2], var0 = p[3], var1 = p[4];
  if (!sc_row_set(mu0, var0)) return;
  const double zz = __ddiv_rn(__dadd_rn(m, -mu0), __dsqrt_rn(var0));
  z = zz != zz ? sc_nan() : zz;
  if (!(pi1 > 0.0 && pi1 < 1.0 && var1 > 0.0 && sc_finite(mu1) && sc_finite(var1))) return;
  const SmParams P{mu0, mu1, var0, var1, __dadd_rn(1.0, -pi1), pi1};
  const double x[1] = {m};
  const bool in[1] = {true};
  double g0[1], g1[1];
  sm_estep<1>(P, x, in, tab, g0, g1);
  prob = g1[0] != g1[0] ? sc_nan() : g1[0];
}

__device__ __forceinline__ bool sc_read_wanted(const SiteCalls& sc, const ReadDesc& rd, const ReadState* __restrict__ st) {
  return rd.read >= sc.read_lo && rd.read < sc.read_hi && st[rd.read].status == 0;
}

// grid (n_reads, ceil((max_N - 1) / 256)): thread j of block (r, c) owns output row c * 256 + j of read descs[r]
__global__ __launch_bounds__(256) void k_scall_short(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                     const uint32_t* __restrict__ segrow_all, SiteCalls sc) {
  __shared__ uint64_t s_exp[dynmath::STRICT_EXP_WORDS];
  const ReadDesc rd = descs[blockIdx.x];
  const int n_seg = (int)rd.N - 1;
  if ((int)(blockIdx.y * 256u) >= n_seg) return;  // block-uniform, like the next one: no thread waits at the barrier below
  if (!sc_read_wanted(sc, rd, st)) return;
  const bool scored = sc.sites && sc.model;
  if (scored) {
    for (int i = threadIdx.x; i < dynmath::STRICT_EXP_WORDS; i += 256) s_exp[i] = sc.exp_tab[i];
    __syncthreads();
  }
  const int T = (int)rd.T;
  const int j = (int)(blockIdx.y * 256u + threadIdx.x);
  if (j >= n_seg) return;
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  const int a = (int)segrow[j];
  const int b = (j + 1 < n_seg) ? (int)segrow[j + 1] : T;
  const int L = b - a;
  const bool inside = L >= 1 && a >= 1 && b <= T;
  if (inside && L > SS_SHORT_MAX) return;  // k_scall_long's row
  double prob = sc_nan(), z = sc_nan();
  if (inside && scored) {
    const uint32_t id = sc.sites[rd.par_off + j];
    if (id < sc.num_sites)  // (DYN_SITE_NONE is above every num_sites)
      sc_evaluate(sc, id, L, xs_chunked_sum(sc.sig + rd.sig_off + (a - 1), L), s_exp, prob, z);  // sample row - 1
  }
  const uint64_t o = rd.seg_off + (uint64_t)j;
  sc.prob[o] = prob;
  sc.z[o] = z;
}

__global__ __launch_bounds__(256) void k_scall_long(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                    const uint32_t* __restrict__ segrow_all, SiteCalls sc) {
  __shared__ uint64_t s_exp[dynmath::STRICT_EXP_WORDS];
  __shared__ double s_p1[256];
  const ReadDesc rd = descs[blockIdx.x];
  if (!sc_read_wanted(sc, rd, st)) return;
  const int T = (int)rd.T, n_seg = (int)rd.N - 1;
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  int any = 0;
  for (int i = tid; i < n_seg; i += 256) {
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    any |= (b - a > SS_SHORT_MAX);
  }
  if (!__syncthreads_or(any)) return;
  const bool scored = sc.sites && sc.model;
  if (scored) {
    for (int i = tid; i < dynmath::STRICT_EXP_WORDS; i += 256) s_exp[i] = sc.exp_tab[i];
    __syncthreads();
  }
  for (int i = 0; i < n_seg; ++i) {  // block-uniform walk over the rows of this read
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    const int L = b - a;
    if (L <= SS_SHORT_MAX || a < 1 || b > T) continue;  // k_scall_short's rows
    const uint64_t o = rd.seg_off + (uint64_t)i;
    const uint32_t id = scored ? sc.sites[rd.par_off + i] : SS_SITE_NONE;  // block-uniform
    if (id >= sc.num_sites) {
      if (tid == 0) {
        sc.prob[o] = sc_nan();
        sc.z[o] = sc_nan();
      }
      continue;
    }
    const double* __restrict__ xs = sc.sig + rd.sig_off + (a - 1);
    const int n_chunks = (L + XS_CHUNK - 1) / XS_CHUNK;
    double acc1 = 0.0;  // lane 0's running total
    for (int c0 = 0; c0 < n_chunks; c0 += 256) {
      const int c = c0 + tid;
      if (c < n_chunks) s_p1[tid] = xs_chunked_sum(xs + c * XS_CHUNK, min(XS_CHUNK, L - c * XS_CHUNK));
      __syncthreads();
      if (tid == 0)
        for (int k = 0; k < min(256, n_chunks - c0); ++k) acc1 = (c0 + k == 0) ? s_p1[k] : __dadd_rn(acc1, s_p1[k]);
      __syncthreads();
    }
    if (tid == 0) {
      double prob, z;
      sc_evaluate(sc, id, L, acc1, s_exp, prob, z);
      sc.prob[o] = prob;
      sc.z[o] = z;
    }
  }
}

// the two launches of launch_site_calls (site_summary.hip); descs in processing order, max_N the largest ReadDesc::N
inline void launch_site_call_kernels(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st, const uint32_t* segrow,
                                     const SiteCalls& sc, hipStream_t s) {
  if (!sc.prob || !sc.z || !sc.sig || n_reads <= 0 || max_N < 2 || sc.read_lo >= sc.read_hi) return;
  if (sc.sites && sc.model && (!sc.exp_tab || (sc.map_keys && !sc.capacity))) return;
  const unsigned chunks = (max_N - 1 + 255) / 256;
  hipLaunchKernelGGL(k_scall_short, dim3((unsigned)n_reads, chunks), dim3(256), 0, s, descs, st, segrow, sc);
  hipLaunchKernelGGL(k_scall_long, dim3((unsigned)n_reads), dim3(256), 0, s, descs, st, segrow, sc);
}

// one thread per staged row: the ids [lo, lo + count) of a sparse table
__global__ __launch_bounds__(256) void k_site_model_scatter(SiteModelScatter ms) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= ms.count) return;
  const double* __restrict__ src = ms.rows + (uint64_t)t * SC_MODEL_FIELDS;
  const uint32_t id = ms.lo + t;  // (lo + count <= num_sites < 2^32: no wrap)
  const bool set = sc_row_set(src[1], src[3]);
  const uint32_t row = set ? sm_find_or_insert(ms.keys, ms.capacity, ms.stats, id) : sm_find(ms.keys, ms.capacity, id);
  if (row == SM_NO_ROW) {
    if (set) atomicAdd(ms.dropped, 1ull);
    return;
  }
  double* __restrict__ dst = ms.model + (uint64_t)row * SC_MODEL_FIELDS;
  for (int f = 0; f < SC_MODEL_FIELDS; ++f) dst[f] = src[f];
}

inline void launch_site_model_scatter_kernel(const SiteModelScatter& ms, hipStream_t s) {
  if (!ms.keys || !ms.capacity || !ms.stats || !ms.model || !ms.rows || !ms.dropped || ms.count == 0) return;
  hipLaunchKernelGGL(k_site_model_scatter, dim3((ms.count + 255u) / 256u), dim3(256), 0, s, ms);
}

__global__ __launch_bounds__(256) void k_site_model_gather(SiteModelGather mg) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= mg.count) return;
  const uint32_t row = sm_find(mg.keys, mg.capacity, mg.lo + t);
  double* __restrict__ dst = mg.out + (uint64_t)t * SC_MODEL_FIELDS;
  for (int f = 0; f < SC_MODEL_FIELDS; ++f) dst[f] = row == SM_NO_ROW ? 0.0 : mg.model[(uint64_t)row * SC_MODEL_FIELDS + f];
}

inline void launch_site_model_gather_kernel(const SiteModelGather& mg, hipStream_t s) {
  if (!mg.keys || !mg.capacity || !mg.model || !mg.out || mg.count == 0) return;
  hipLaunchKernelGGL(k_site_model_gather, dim3((mg.count + 255u) / 256u), dim3(256), 0, s, mg);
}

}  // namespace dynk
