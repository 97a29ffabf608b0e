// auto_guide.hip -- the pre-pass of dyn_batch_auto_guide: k_auto_guide derives every read's guide on the device from the signal
// and the emission parameters the batch already holds there (definition and per-cell arithmetic: auto_guide_kernels.hpp).
// Modelled on band_read (band_reads.hip): the same band-column addressing (B = 2 hw + 3 band columns per row incl. the two
// guards, start_t = c_t - hw, band column b <-> lattice column n = start_t + b - 1, a shift >= 0 of any size between rows, a
// neighbour row's column outside [0, B) reads as -inf), the same THREADS x CPT shapes picked from B, one workgroup per read,
// reads taken off a queue. What differs:
//   rows        two LDS rows (vE, vM of row t - 1) and nothing else: no arena, no exp table, no logPlus
//   centre      not read from a guide but made here: the previous row's argmax (ag_take / ag_merge) and ag_centre; thread 0
//               stores it as guide[t - 1]
//   argmax      a reduction on the critical path of every row. Each thread folds its own cells as it produces them (ascending
//               columns), the wave finishes with a 6-step xor butterfly of (value, column) in registers -- every lane ends with
//               the wave's result. 64-thread shapes stop there. The 256-thread shape has its four waves' lanes 0 write their
//               pair next to the row store, between the row's two barriers, and every thread folds the four pairs after the
//               second: one LDS exchange per row and no barrier of its own
// ag_merge is symmetric and only values above -inf enter, so the butterfly gives the ascending scan's result in every lane.
#include "auto_guide_kernels.hpp"

namespace dynk {

using dynmath::NEG_INF;

namespace {

__host__ __device__ constexpr int ag_row_stride(int B) { return (B + 1) & ~1; }  // doubles per LDS row: rows stay 16 B aligned

// one read; lds: [2 rows of `stride` doubles | 4 doubles | 4 ints | 4 ints of control]
template <int THREADS, int CPT>
__device__ void auto_guide_read(const ReadDesc& rd, const AutoGuideArgs& a, double* s_rows, int stride, double* s_pv, int* s_pn) {
  constexpr int UNROLL = CPT <= 4 ? CPT : 1;
  constexpr int WAVES = THREADS / 64;
  const int tid = threadIdx.x;
  const int T = (int)rd.T, N = (int)rd.N, hw = a.bw, B = 2 * hw + 3;
  const double m1 = a.m1, e2 = a.e2;
  const double* __restrict__ sg = a.sig + rd.sig_off;
  int32_t* __restrict__ gd = a.guide + rd.sig_off;   // guide[t - 1], t = 1 .. T - 1: the read's own samples
  const Emis* __restrict__ pr = a.par + rd.par_off;  // entry n - 1 <-> lattice column n
  double* pE = s_rows;           // vE of row t - 1
  double* pM = s_rows + stride;  // vM of row t - 1
  auto at = [&](const double* row, int c) { return (c >= 0 && c < B) ? row[c] : NEG_INF; };
#pragma unroll UNROLL
  for (int k = 0; k < CPT; ++k) {
    const int c = tid + k * THREADS;
    if (c < B) {
      pE[c] = (c == hw + 1) ? 0.0 : NEG_INF;  // (0, 0): start_0 = -hw
      pM[c] = NEG_INF;
    }
  }
  __syncthreads();
  int centre = 0, best = 0, start_prev = -hw;  // row 0's argmax is its one cell
  for (int t = 1; t < T; ++t) {
    centre = ag_centre(centre, best, t, T, N);
    if (tid == 0) gd[t - 1] = (int32_t)centre;
    const int start = centre - hw;
    const int n_lo = start > 1 ? start : 1, n_hi = (centre + hw + 1 < N) ? centre + hw + 1 : N;
    const int shift = start - start_prev;  // >= 0
    start_prev = start;
    const double x = sg[t - 1];
    double oE[CPT], oM[CPT];
    double bv = NEG_INF;
    int bn = AG_NONE;
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      double vE = NEG_INF, vM = NEG_INF;
      if (c < B) {
        const int n = start + c - 1;
        if (c >= 1 && c <= 2 * hw + 1 && n >= n_lo && n < n_hi) {
          const int cp = c + shift;  // band column of lattice column n in row t - 1
          ag_cell(at(pE, cp - 1), at(pE, cp), at(pM, cp), dynmath::log_normal_pdf_strict(x, pr[n - 1]), m1, e2, vE, vM);
          ag_take(bv, bn, ag_s(vE, vM), n);
        }
      }
      oE[k] = vE;
      oM[k] = vM;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const double ov = __shfl_xor(bv, d);
      const int on = __shfl_xor(bn, d);
      ag_merge(bv, bn, ov, on);
    }
    __syncthreads();
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      if (c < B) {
        pE[c] = oE[k];
        pM[c] = oM[k];
      }
    }
    if (WAVES > 1 && (tid & 63) == 0) {
      s_pv[tid >> 6] = bv;
      s_pn[tid >> 6] = bn;
    }
    __syncthreads();
    if (WAVES > 1) {
      bv = s_pv[0];
      bn = s_pn[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) ag_merge(bv, bn, s_pv[w], s_pn[w]);
    }
    best = bn == AG_NONE ? -1 : bn;
  }
  __syncthreads();
}

}  // namespace

// one workgroup takes reads off a queue until it is empty
template <int THREADS, int CPT>
__global__ __launch_bounds__(THREADS) void k_auto_guide(const AutoGuideArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ag_lds[];
  const int stride = ag_row_stride(2 * a.bw + 3);
  double* s_rows = reinterpret_cast<double*>(ag_lds);
  double* s_pv = s_rows + 2 * stride;
  int* s_pn = reinterpret_cast<int*>(s_pv + 4);
  int* s_ctl = s_pn + 4;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[0] = (int)atomicAdd(a.head, 1u);
    __syncthreads();
    const int k = s_ctl[0];
    // the guide rescue (launch_rescue_select) hands over the list of the reads to guide and its length on the device
    const bool listed = a.active != nullptr;
    if (k >= (listed ? (int)*a.n_active : a.n_reads)) break;
    const ReadDesc rd = a.descs[listed ? a.active[k] : (uint32_t)k];
    auto_guide_read<THREADS, CPT>(rd, a, s_rows, stride, s_pv, s_pn);
  }
}

namespace {
// shapes, narrowest first: B = 2 hw + 3 <= THREADS * CPT (band_reads.hip's); groups: an upper bound on the workgroups per CU
struct Shape { int threads, cpt, groups; };
constexpr Shape SHAPES[] = {{64, 1, 16}, {64, 4, 16}, {256, 16, 2}};
const Shape& shape_of(int bw) {
  const int B = 2 * bw + 3;
  for (const Shape& s : SHAPES)
    if (B <= s.threads * s.cpt) return s;
  return SHAPES[2];
}
size_t lds_bytes(int bw) { return 2 * (size_t)ag_row_stride(2 * bw + 3) * 8 + 32 + 16 + 16; }
template <int THREADS, int CPT>
hipError_t launch_shape(const AutoGuideArgs& a, int n_groups, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024) {  // (a wide window: the request exceeds the default dynamic-LDS limit)
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_auto_guide<THREADS, CPT>),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((k_auto_guide<THREADS, CPT>), dim3(n_groups), dim3(THREADS), lds, s, a);
  return hipGetLastError();
}
}  // namespace

int auto_guide_groups_per_cu(int bw) {
  const int by_lds = (int)((150 * 1024) / lds_bytes(bw));
  const int by_waves = shape_of(bw).groups;
  return by_lds < 1 ? 1 : by_lds < by_waves ? by_lds : by_waves;
}

hipError_t launch_auto_guide(const AutoGuideArgs& a, int n_groups, hipStream_t s) {
  if (a.n_reads <= 0 || n_groups <= 0) return hipSuccess;
  if (a.bw < 1 || a.bw > WIDE_MAX_HALF_BAND || !a.guide || !a.head || (a.active && !a.n_active)) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(a.head, 0, 4, s)) return e;
  const size_t lds = lds_bytes(a.bw);
  const Shape& sh = shape_of(a.bw);
  if (sh.cpt == 1) return launch_shape<64, 1>(a, n_groups, lds, s);
  if (sh.threads == 64) return launch_shape<64, 4>(a, n_groups, lds, s);
  return launch_shape<256, 16>(a, n_groups, lds, s);
}

}  // namespace dynk
