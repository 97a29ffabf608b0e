// kmer_summary_kernels.hpp -- the per-k-mer level summary of a run (dyn_aligner_set_kmer_summary): for every k-mer code the
// number of segments and samples the run aligned to it and the sums of x and x^2 over those samples, as EXACT INTEGERS.
// Included by kmer_summary.hip (launch_kmer_summary) and by tests/device_math/kmer_summary.hip, which feeds the launch path
// arrays built on the host and compares every integer with a Python-int restatement (tests/test_gpu_kmer_summary.py).
// The kernels are ordinary (non-inline) definitions: one translation unit per binary includes this file.
//
// Definition. Output row j of an ok read covers lattice rows [segrow[j], segrow[j+1]) (the last
// one up to T), i.e. samples row - 1 of the signal the read queue aligned, and belongs to k-mer code kmers[par_off + j].
//   S1, S2   the chunked sums of event_stats.hip (chunks of 64 from the segment's first sample, each left to right, the chunk
//            sums left to right; one IEEE fp64 operation each, no contraction) of x and of __dmul_rn(x, x)
//   q1, q2   rint(S1 * 2^40), rint(S2 * 2^40) as exact integers (ties to even; the scaling by a power of two is exact)
//   skipped  a segment with S2 >= 2^64 or a non-finite S1 / S2 (|S1| <= sqrt(L S2) bounds q1 with it): counted, not added
// Per k-mer six u64: n_segments, n_samples, Q1 = sum q1 and Q2 = sum q2 as 128-bit two's complement (low limb, high limb).
// Integer addition commutes: the atomics below may land in any order and the totals are the same bits whatever the launch
// path, the merging of tickets or the number of ranks. No float atomics, no sort.
// Two kernels, split like k_event_short / k_event_long at KS_SHORT_MAX samples:
//   k_ksum_short  one thread per OUTPUT row (not per lattice row): block (read, chunk of 256 rows)
//   k_ksum_long   one 256-thread block per read that has a longer segment: lanes sum chunks in parallel, lane 0 adds the
//                 chunk sums in order (the chunk loop wraps beyond 256 chunks, segments above 16 384 samples)
// The chunked sums, the double -> 128-bit conversion and the 128-bit add are exact_sum_kernels.hpp (shared with the per-site
// summary, site_summary_kernels.hpp).
// Footprint: 256 threads, 4 KB of static LDS (k_ksum_long), no scratch -- they run beside a resident workgroup.
#pragma once

#include "exact_sum_kernels.hpp"
#include "nt_kernels.hpp"

namespace dynk {

constexpr int KS_SHORT_MAX = 256;
constexpr int KS_CHUNK = XS_CHUNK;
constexpr int KS_FIELDS = 6;  // per k-mer: n_segments, n_samples, q1_lo, q1_hi, q2_lo, q2_hi
constexpr int KS_TOTALS = 4;  // reads_ok, segments, samples, skipped_segments

// does the definition keep the segment? (NaN fails the first comparison)
__device__ __forceinline__ bool ks_kept(double s1, double s2) {
  return s2 < 18446744073709551616.0 && s2 >= 0.0 && fabs(s1) <= 1.7976931348623157e308;
}

// one segment into its k-mer's cell; returns false when the definition skips it
__device__ __forceinline__ bool ks_accumulate(const KmerSummary& ks, int32_t code, int L, double s1, double s2) {
  if (!ks_kept(s1, s2)) return false;
  unsigned long long* cell = ks.acc + (uint64_t)code * KS_FIELDS;
  atomicAdd(cell, 1ull);
  atomicAdd(cell + 1, (unsigned long long)L);
  unsigned long long lo, hi;
  xs_to_i128(rint(__dmul_rn(s1, 1099511627776.0)), lo, hi);
  xs_add128(cell + 2, lo, hi);
  xs_to_i128(rint(__dmul_rn(s2, 1099511627776.0)), lo, hi);
  xs_add128(cell + 4, lo, hi);
  return true;
}

__device__ __forceinline__ bool ks_read_wanted(const KmerSummary& ks, const ReadDesc& rd, const ReadState* __restrict__ st) {
  return rd.read >= ks.read_lo && rd.read < ks.read_hi && st[rd.read].status == 0;
}

// grid (n_reads, ceil((max_N - 1) / 256)): thread j of block (r, c) owns output row c * 256 + j of read descs[r]
__global__ __launch_bounds__(256) void k_ksum_short(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                    const uint32_t* __restrict__ segrow_all, KmerSummary ks) {
  const ReadDesc rd = descs[blockIdx.x];
  const int n_seg = (int)rd.N - 1;
  if ((int)(blockIdx.y * 256u) >= n_seg) return;
  if (!ks_read_wanted(ks, rd, st)) return;
  const int T = (int)rd.T;
  const int j = (int)(blockIdx.y * 256u + threadIdx.x);
  unsigned long long n_kept = 0, n_samp = 0, n_skip = 0;
  if (j < n_seg) {
    const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
    const int a = (int)segrow[j];
    const int b = (j + 1 < n_seg) ? (int)segrow[j + 1] : T;
    const int L = b - a;
    const int32_t code = ks.kmers[rd.par_off + j];
    if (L >= 1 && L <= KS_SHORT_MAX && a >= 1 && b <= T) {
      if ((uint32_t)code < ks.num_kmers) {
        double s1, s2;
        xs_chunked_sums(ks.sig + rd.sig_off + (a - 1), L, s1, s2);  // sample row - 1
        if (ks_accumulate(ks, code, L, s1, s2)) {
          n_kept = 1;
          n_samp = (unsigned long long)L;
        } else {
          n_skip = 1;
        }
      } else {
        n_skip = 1;
      }
    }
  }
  n_kept = xs_wave_sum(n_kept);
  n_samp = xs_wave_sum(n_samp);
  n_skip = xs_wave_sum(n_skip);
  if ((threadIdx.x & (warpSize - 1)) == 0) {
    if (n_kept) atomicAdd(ks.totals + 1, n_kept);
    if (n_samp) atomicAdd(ks.totals + 2, n_samp);
    if (n_skip) atomicAdd(ks.totals + 3, n_skip);
  }
  if (blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(ks.totals, 1ull);  // reads_ok
}

__global__ __launch_bounds__(256) void k_ksum_long(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                   const uint32_t* __restrict__ segrow_all, KmerSummary ks) {
  __shared__ double s_p1[256];
  __shared__ double s_p2[256];
  const ReadDesc rd = descs[blockIdx.x];
  if (!ks_read_wanted(ks, rd, st)) return;
  const int T = (int)rd.T, n_seg = (int)rd.N - 1;
  const int tid = threadIdx.x;
  const uint32_t* __restrict__ segrow = segrow_all + rd.seg_off;
  int any = 0;
  for (int i = tid; i < n_seg; i += 256) {
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    any |= (b - a > KS_SHORT_MAX);
  }
  if (!__syncthreads_or(any)) return;
  for (int i = 0; i < n_seg; ++i) {  // block-uniform walk over the segments of this read
    const int a = (int)segrow[i], b = (i + 1 < n_seg) ? (int)segrow[i + 1] : T;
    const int L = b - a;
    if (L <= KS_SHORT_MAX || a < 1 || b > T) continue;
    const double* __restrict__ xs = ks.sig + rd.sig_off + (a - 1);
    const int n_chunks = (L + KS_CHUNK - 1) / KS_CHUNK;
    double acc1 = 0.0, acc2 = 0.0;  // lane 0's running totals
    for (int c0 = 0; c0 < n_chunks; c0 += 256) {
      const int c = c0 + tid;
      if (c < n_chunks) {
        double p1, p2;
        xs_chunked_sums(xs + c * KS_CHUNK, min(KS_CHUNK, L - c * KS_CHUNK), p1, p2);
        s_p1[tid] = p1;
        s_p2[tid] = p2;
      }
      __syncthreads();
      if (tid == 0)
        for (int k = 0; k < min(256, n_chunks - c0); ++k) {
          acc1 = (c0 + k == 0) ? s_p1[k] : __dadd_rn(acc1, s_p1[k]);
          acc2 = (c0 + k == 0) ? s_p2[k] : __dadd_rn(acc2, s_p2[k]);
        }
      __syncthreads();
    }
    if (tid == 0) {
      const int32_t code = ks.kmers[rd.par_off + i];
      if ((uint32_t)code < ks.num_kmers && ks_accumulate(ks, code, L, acc1, acc2)) {
        atomicAdd(ks.totals + 1, 1ull);
        atomicAdd(ks.totals + 2, (unsigned long long)L);
      } else {
        atomicAdd(ks.totals + 3, 1ull);
      }
    }
  }
}

// the two launches of launch_kmer_summary (kmer_summary.hip); descs in processing order, max_N the largest ReadDesc::N
inline void launch_kmer_summary_kernels(const ReadDesc* descs, int n_reads, uint32_t max_N, const ReadState* st,
                                        const uint32_t* segrow, const KmerSummary& ks, hipStream_t s) {
  if (!ks.acc || n_reads <= 0 || max_N < 2 || ks.read_lo >= ks.read_hi) return;
  const unsigned chunks = (max_N - 1 + 255) / 256;
  hipLaunchKernelGGL(k_ksum_short, dim3((unsigned)n_reads, chunks), dim3(256), 0, s, descs, st, segrow, ks);
  hipLaunchKernelGGL(k_ksum_long, dim3((unsigned)n_reads), dim3(256), 0, s, descs, st, segrow, ks);
}

}  // namespace dynk
