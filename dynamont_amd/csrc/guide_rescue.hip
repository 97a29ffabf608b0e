// guide_rescue.hip -- the two small kernels of the guide rescue (guide_rescue_kernels.hpp): k_rescue_select turns the diagonal
// band margins of a job's reads into the per-read code and the list of the descriptors to re-align inside a self-made guide;
// k_rescue_merge, behind the rescue alignment, moves the answer of every rescue that ended ok over the plain one.
// Both hand their results to LATER launches on the same stream only: no word is exchanged inside a launch.
#include "guide_rescue_kernels.hpp"

namespace dynk {

namespace {
constexpr int SEL_THREADS = 256;
}

// ONE workgroup. The table is walked in chunks of SEL_THREADS descriptors; within a chunk an inclusive scan of the flags in LDS
// gives every flagged descriptor its place behind the chunks before it: the list is in descriptor order whatever the timing.
__global__ __launch_bounds__(SEL_THREADS) void k_rescue_select(const RescueSelect r) {
  __shared__ uint32_t s_scan[SEL_THREADS];
  __shared__ uint32_t s_base;
  const int tid = (int)threadIdx.x;
  if (tid == 0) s_base = 0u;
  __syncthreads();
  for (int k0 = 0; k0 < r.n_reads; k0 += SEL_THREADS) {
    const int k = k0 + tid;
    uint8_t c = 0;
    uint32_t read = 0;
    if (k < r.n_reads) {
      const ReadDesc rd = r.descs[k];
      read = rd.read;
      c = rescue_decide(r.st[read].status, rd.N, rd.T, r.low[read], r.high[read], r.min_margin, r.max_T);
    }
    const uint32_t flag = c == 1 ? 1u : 0u;
    s_scan[tid] = flag;
    __syncthreads();
    for (int d = 1; d < SEL_THREADS; d <<= 1) {
      const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
      __syncthreads();
      s_scan[tid] += add;
      __syncthreads();
    }
    const uint32_t base = s_base;
    if (flag) r.list[base + s_scan[tid] - 1u] = (uint32_t)k;  // base + (inclusive - 1) < the descriptors seen so far <= n_reads
    if (c) r.code[read] = c;
    __syncthreads();  // everybody has read s_base and its own s_scan entry
    if (tid == SEL_THREADS - 1) s_base = base + s_scan[tid];
    __syncthreads();
  }
  if (tid == 0) *r.n_list = s_base;
}

hipError_t launch_rescue_select(const RescueSelect& r, hipStream_t s) {
  if (!r.code || !r.list || !r.n_list || (r.n_reads > 0 && (!r.descs || !r.st || !r.low || !r.high))) return hipErrorInvalidValue;
  // (with no descriptor the kernel still writes the length, 0: the launches behind it read it)
  hipLaunchKernelGGL(k_rescue_select, dim3(1), dim3(SEL_THREADS), 0, s, r);
  return hipGetLastError();
}

// block k owns descriptor list[k]. A rescue that ended ok: its state, its segment rows (N - 1 entries) and its path rows from
// the first border on (the rows the traceback wrote, and the only ones anything behind it reads) replace the plain ones. One that
// failed: nothing is copied, the code becomes 3 and the counts of the attempt are cleared.
__global__ __launch_bounds__(256) void k_rescue_merge(const RescueMerge r) {
  if (blockIdx.x >= *r.n_list) return;
  const uint32_t idx = r.list[blockIdx.x];
  if (idx >= (uint32_t)r.n_reads) return;
  const ReadDesc rd = r.descs[idx];
  const ReadState s_in = r.st_in[rd.read];
  if (s_in.status != 0) {
    if (threadIdx.x == 0) {
      r.code[rd.read] = RESCUE_FAILED;
      r.rounds[rd.read] = 0u;
      r.converged[rd.read] = 0u;
    }
    return;
  }
  const int T = (int)rd.T, n_seg = (int)rd.N - 1;  // (a flagged read has N >= 2)
  const uint32_t* __restrict__ seg_in = r.segrow_in + rd.seg_off;
  const int first = n_seg > 0 ? (int)seg_in[0] : T;
  const double* __restrict__ pp_in = r.pp_in + rd.path_off;
  const uint32_t* __restrict__ pn_in = r.pathn_in + rd.path_off;
  double* pp = r.pp + rd.path_off;
  uint32_t* pn = r.pathn + rd.path_off;
  uint32_t* seg = r.segrow + rd.seg_off;
  for (int t = (first > 1 ? first : 1) + (int)threadIdx.x; t < T; t += 256) {
    pp[t] = pp_in[t];
    pn[t] = pn_in[t];
  }
  for (int j = (int)threadIdx.x; j < n_seg; j += 256) seg[j] = seg_in[j];
  if (threadIdx.x == 0) {
    r.st[rd.read] = s_in;
    r.code[rd.read] = RESCUE_DONE;
    if (r.single) {
      r.rounds[rd.read] = 1u;
      r.converged[rd.read] = 0u;
    }
  }
}

hipError_t launch_rescue_merge(const RescueMerge& r, hipStream_t s) {
  if (r.n_reads <= 0) return hipSuccess;
  if (!r.descs || !r.list || !r.n_list || !r.st_in || !r.pp_in || !r.pathn_in || !r.segrow_in || !r.st || !r.pp || !r.pathn || !r.segrow ||
      !r.code || !r.rounds || !r.converged)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rescue_merge, dim3((unsigned)r.n_reads), dim3(256), 0, s, r);
  return hipGetLastError();
}

}  // namespace dynk
