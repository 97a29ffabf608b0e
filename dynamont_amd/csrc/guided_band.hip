// guided_band.hip -- the guided band (dyn_batch_set_guide): the reference's algorithm inside a narrow window that follows a
// per-read guide path instead of the fixed diagonal. Modelled on wide_read (wide_band.hip): the reference's band-column
// addressing, the reference's OWN arithmetic in every cell (dp_math_strict.hpp), the same per-row outputs (pp, pathn, segrow,
// ReadState), so that launch_segments / k_median / k_final follow unchanged. What differs (guided_band_kernels.hpp):
//   window      centre(t) = guide[sig_off + t - 1] (centre(0) = 0), bw = the batch's half width, not clamped to N / 2
//   shift       start_t - start_{t-1} >= 0 of ANY size; a neighbour row's column outside [0, B) reads as -inf
//   boundaries  at the lattice cells themselves: backward seed (T-1, N-1), forward / Viterbi seed (0, 0), Zb at (0, 0),
//               Zf at (T-1, N-1); a cell outside its row's window is -inf, and the read then fails the reference's own
//               Z check (DYN_READ_Z_MISMATCH): an infeasible guide costs that read only
//   geometry    THREADS x CPT shapes picked per launch from B = 2 bw + 3; the four LDS rows are sized from B (dynamic LDS,
//               every carve a multiple of 16 B), the per-thread row registers by CPT; shapes of CPT <= 4 are fully unrolled
//               (registers, no scratch), several workgroups share a CU
//   Z only      nothing of the lattice is stored: the backward rows live in LDS, no arena
//   train       (dyn_batch_train_guided) the backward sweep stores bE / bM (16 B per cell, nothing else in the arena); the
//               forward sweep forms LPM / LPE as the align job does and, instead of posterior-Viterbi and the traceback, adds
//               g = exp(LPM) + exp(LPE) into the read's per-column sums (w, s1, s2) of TrainBuffers. Scheme: a per-row
//               read-modify-write of the column sums in global memory -- the lanes of a row own distinct lattice columns and
//               the row's barrier separates it from the next row, whose owner of a column may be another lane after a shift
//               of any size. Nothing is held across rows, so there is nothing to flush and no index depends on the shift:
//               every access is entry n - 1 of a cell's own column n in [1, N). Each column's sum is formed in ascending t,
//               without atomics: the same bits whichever workgroup takes the read. Two LDS rows (the forward rows) only.
// A diagonal guide at bw = min(band / 2, N / 2) is the reference's band: the results are the reference's bit for bit.
#include "guided_band_kernels.hpp"

#include "dp_math_strict.hpp"

namespace dynk {

using dynmath::NEG_INF;

namespace {

constexpr uint32_t GBM_NONE = 0xffffffffu;  // DYN_BAND_MARGIN_NONE

__host__ __device__ constexpr int guided_row_stride(int B) { return (B + 1) & ~1; }  // doubles per LDS row: rows stay 16 B aligned

// one read; lds: [STRICT_EXP_WORDS u64 | 4 rows (TRAIN: 2) of `stride` doubles | 4 ints]
// TRAIN: the statistics pass instead of posterior-Viterbi + traceback. CALC: align(calc_probabilities = true).
template <int THREADS, int CPT, bool CALC, bool TRAIN>
__device__ void guided_read(const ReadDesc& rd, const GuidedArgs& a, double* __restrict__ bE, double* __restrict__ bM,
                            float* __restrict__ lp, uint8_t* __restrict__ bit, double* s_rows, int stride, const uint64_t* s_exp,
                            int* s_bad) {
  constexpr int UNROLL = CPT <= 4 ? CPT : 1;
  const int tid = threadIdx.x;
  const int T = (int)rd.T, N = (int)rd.N, bw = a.bw, B = 2 * bw + 3;
  const double m1 = a.m1, e2 = a.e2;
  const double* __restrict__ sg = a.sig + rd.sig_off;
  const int32_t* __restrict__ gd = a.guide + rd.sig_off;  // centre(t) = gd[t - 1], t >= 1
  const Emis* __restrict__ pr = a.par + rd.par_off;        // entry n - 1 <-> lattice column n
  double* nxE = s_rows;               // backward: row t + 1;  forward: fE of row t - 1
  double* nxM = s_rows + stride;      //                         forward: fM of row t - 1
  double* pvE = TRAIN ? nullptr : s_rows + 2 * stride;  // forward: vE of row t - 1 (TRAIN: no such rows in LDS)
  double* pvM = TRAIN ? nullptr : s_rows + 3 * stride;  // forward: vM of row t - 1
  if (tid == 0) *s_bad = 0;
  auto at = [&](const double* row, int c) { return (c >= 0 && c < B) ? row[c] : NEG_INF; };  // guard columns and beyond: -inf
  auto centre = [&](int t) { return t > 0 ? (int)gd[t - 1] : 0; };

  // ---- backward: t = T-2 .. 0 ----
  {
    const int c_seed = (N - 1) - (centre(T - 1) - bw) + 1;  // band column of (T-1, N-1); outside 1 .. 2 bw + 1: no seed
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      if (c < B) {
        const double v = (c == c_seed && c >= 1 && c <= 2 * bw + 1) ? 0.0 : NEG_INF;
        nxE[c] = v;
        nxM[c] = NEG_INF;
        if (CALC || TRAIN) {
          bE[(size_t)(T - 1) * B + c] = v;
          bM[(size_t)(T - 1) * B + c] = NEG_INF;
        }
      }
    }
  }
  __syncthreads();
  int bad = 0;
  int start_next = centre(T - 1) - bw;
  for (int t = T - 2; t >= 0; --t) {
    const int mid = centre(t), start = mid - bw;
    const int n_lo = start > 0 ? start : 0, n_hi = (mid + bw + 1 < N) ? mid + bw + 1 : N;
    const int shift = start_next - start;  // start_{t+1} - start_t >= 0
    start_next = start;
    const double x = sg[t];
    bad |= !(__builtin_fabs(x) <= 1.7976931348623157e308);
    double oE[CPT], oM[CPT];
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      double ext = NEG_INF, bm = NEG_INF;
      if (c < B) {
        const int n = start + c - 1;
        if (c >= 1 && c <= 2 * bw + 1 && n >= n_lo && n < n_hi) {
          const int cn = c - shift;  // band column of lattice column n in row t + 1
          if (n + 1 < N) ext = (at(nxM, cn + 1) + dynmath::log_normal_pdf_strict(x, pr[n])) + m1;
          if (n > 0) {
            const double score = dynmath::log_normal_pdf_strict(x, pr[n - 1]);
            const double e_next = at(nxE, cn);
            bm = e_next + score;
            ext = dynmath::log_plus_strict(ext, (e_next + score) + e2, s_exp);
          }
        }
      }
      oE[k] = ext;
      oM[k] = bm;
    }
    __syncthreads();
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      if (c < B) {
        nxE[c] = oE[k];
        nxM[c] = oM[k];
        if (CALC || TRAIN) {
          bE[(size_t)t * B + c] = oE[k];
          bM[(size_t)t * B + c] = oM[k];
        }
      }
    }
    __syncthreads();
  }
  if (bad) *s_bad = 1;
  const double Zb_raw = nxE[bw + 1];  // (0, 0): start_0 = -bw
  __syncthreads();
  const double Zb = *s_bad ? NEG_INF : Zb_raw;  // an infinite / NaN sample: "alignment scores do not match"

  // ---- forward + posterior + posterior-Viterbi + decision bit, t = 1 .. T-1 ----
#pragma unroll UNROLL
  for (int k = 0; k < CPT; ++k) {
    const int c = tid + k * THREADS;
    if (c < B) {
      const double v = (c == bw + 1) ? 0.0 : NEG_INF;  // (0, 0)
      nxE[c] = v;
      nxM[c] = NEG_INF;
      if (!TRAIN) {
        pvE[c] = v;
        pvM[c] = NEG_INF;
      }
    }
  }
  // TRAIN: the read's column sums start at 0 (entry n - 1 <-> lattice column n, N - 1 entries). Not __restrict__: a column's
  // word is written by one lane and read by another in the next row
  double* cw = TRAIN ? a.tr.col_w + rd.par_off : nullptr;
  double* cs1 = TRAIN ? a.tr.col_s1 + rd.par_off : nullptr;
  double* cs2 = TRAIN ? a.tr.col_s2 + rd.par_off : nullptr;
  if (TRAIN) {
    for (int n = tid; n < N - 1; n += THREADS) cw[n] = cs1[n] = cs2[n] = 0.0;
  }
  __syncthreads();
  int start_prev = -bw;
  for (int t = 1; t < T; ++t) {
    const int mid = centre(t), start = mid - bw;
    const int n_lo = start > 1 ? start : 1, n_hi = (mid + bw + 1 < N) ? mid + bw + 1 : N;  // forward never fills n = 0
    const int shift = start - start_prev;  // >= 0
    start_prev = start;
    const double x = sg[t - 1];
    double ofE[CPT], ofM[CPT], ovE[CALC ? CPT : 1], ovM[CALC ? CPT : 1];
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      double fM = NEG_INF, fE = NEG_INF, vM = NEG_INF, vE = NEG_INF;
      if (c < B) {
        const int n = start + c - 1;
        if (c >= 1 && c <= 2 * bw + 1 && n >= n_lo && n < n_hi) {
          const int cp = c + shift;  // band column of lattice column n in row t - 1
          const double score = dynmath::log_normal_pdf_strict(x, pr[n - 1]);
          fM = (at(nxE, cp - 1) + score) + m1;
          fE = dynmath::log_plus_strict((at(nxM, cp) + score) + 0.0, (at(nxE, cp) + score) + e2, s_exp);
          if (TRAIN) {
            // n in [max(start, 1), min(centre + bw + 1, N)): entry n - 1 lies in the read's N - 1 entries whatever the shift.
            // This lane alone owns column n in this row; the barrier below orders it against the next row's owner.
            const size_t cell = (size_t)t * B + c;
            const double LPM = (fM + bM[cell]) - Zb, LPE = (fE + bE[cell]) - Zb;
            const double g = exp(LPM) + exp(LPE);
            cw[n - 1] += g;
            cs1[n - 1] += g * x;
            cs2[n - 1] += (g * x) * x;
          } else if (CALC) {
            const size_t cell = (size_t)t * B + c;
            const double LPM = (fM + bM[cell]) - Zb, LPE = (fE + bE[cell]) - Zb;
            vM = at(pvE, cp - 1) + LPM;
            const double um = at(pvM, cp), ue = at(pvE, cp);
            vE = (um < ue ? ue : um) + LPE;  // std::max
            lp[2 * cell] = (float)LPM;
            lp[2 * cell + 1] = (float)LPE;
            bit[cell] = (vE == um + LPE) ? 1 : 0;
          }
        }
      }
      ofE[k] = fE;
      ofM[k] = fM;
      if (CALC) {
        ovE[k] = vE;
        ovM[k] = vM;
      }
    }
    __syncthreads();
#pragma unroll UNROLL
    for (int k = 0; k < CPT; ++k) {
      const int c = tid + k * THREADS;
      if (c < B) {
        nxE[c] = ofE[k];
        nxM[c] = ofM[k];
        if (CALC) {
          pvE[c] = ovE[k];
          pvM[c] = ovM[k];
        }
      }
    }
    __syncthreads();
  }
  const int c_last = (N - 1) - start_prev + 1;  // band column of (T-1, N-1) (T = 1: row 0)
  const double Zf = (c_last >= 1 && c_last <= 2 * bw + 1) ? nxE[c_last] : NEG_INF;
  // Z check (NT_aligner_api.cpp:285-291)
  const double size = (double)((uint64_t)T * (uint64_t)B);
  const bool ok = !(isinf(Zf) || isinf(Zb)) && !(__builtin_fabs(Zf - Zb) / size > 1e-8);
  int status = ok ? 0 : a.z_fail_status;
  uint32_t n_seg = 0;
  __syncthreads();

  // ---- decodeMAP: one lane walks the decision bits from (T-1, N-1) in state E ----
  if (CALC && ok) {
    if (tid == 0) {
      double* __restrict__ pp = a.tb.pp + rd.path_off;
      uint32_t* __restrict__ pathn = a.tb.pathn + rd.path_off;
      uint32_t* __restrict__ segrow = a.tb.segrow + rd.seg_off;
      int t = T - 1, n = N - 1;
      bool isM = false, inside = true;
      while (t > 0 && n > 0) {
        const int c = n - (centre(t) - bw) + 1;
        if (c < 1 || c > 2 * bw + 1) {  // (a path of finite value never leaves the window)
          inside = false;
          break;
        }
        const size_t cell = (size_t)t * B + c;
        if (isM) {
          pp[t] = exp((double)lp[2 * cell]);
          pathn[t] = (uint32_t)n | 0x80000000u;
          segrow[n - 1] = (uint32_t)t;
          --t;
          --n;
          isM = false;
        } else {
          pp[t] = exp((double)lp[2 * cell + 1]);
          pathn[t] = (uint32_t)n;
          isM = bit[cell] != 0;
          --t;
        }
      }
      *s_bad = (inside && t == 0 && n == 0) ? 0 : 2;
    }
    __syncthreads();
    if (*s_bad == 2) status = 7;  // DYN_READ_INTERNAL
    else n_seg = rd.N - 1;
  }
  if (TRAIN && tid == 0 && ok) {
    // expected transition counts: every path makes N - 1 moves and T - 1 - 2 (N - 1) extensions
    a.tr.trans[2 * rd.read] = (double)(N - 1);
    a.tr.trans[2 * rd.read + 1] = (double)(T - 1 - 2 * (N - 1));
  }
  if (tid == 0) {
    ReadState s;
    s.Zb = Zb;
    s.Zf = Zf;
    s.status = status;
    s.n_segments = n_seg;
    a.st[rd.read] = s;
  }
  __syncthreads();
}

}  // namespace

// one workgroup takes reads off a queue until it is empty; its lattice arena (jobs 1 and 2) holds one read at a time
template <int THREADS, int CPT, bool CALC, bool TRAIN>
__global__ __launch_bounds__(THREADS) void k_guided_reads(const GuidedArgs a) {
  extern __shared__ __attribute__((aligned(16))) char g_lds[];
  const int stride = guided_row_stride(2 * a.bw + 3);
  uint64_t* s_exp = reinterpret_cast<uint64_t*>(g_lds);
  double* s_rows = reinterpret_cast<double*>(g_lds + dynmath::STRICT_EXP_WORDS * 8);
  int* s_ctl = reinterpret_cast<int*>(s_rows + (TRAIN ? 2 : 4) * stride);  // [0] next read, [1] s_bad
  for (int i = threadIdx.x; i < dynmath::STRICT_EXP_WORDS; i += THREADS) s_exp[i] = a.exp_tab[i];
  char* arena = a.arena + (size_t)blockIdx.x * a.arena_bytes;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[0] = (int)atomicAdd(a.head, 1u);
    __syncthreads();
    const int k = s_ctl[0];
    // a refinement round (launch_guide_refine) hands over the list of the reads still to align and its length on the device
    if (k >= (a.active ? (int)*a.n_active : a.n_reads)) break;
    const ReadDesc rd = a.descs[a.active ? a.active[k] : (uint32_t)k];
    const size_t cells = (size_t)rd.T * (size_t)(2 * a.bw + 3);
    double* bE = reinterpret_cast<double*>(arena);
    double* bM = bE + cells;
    float* lp = reinterpret_cast<float*>(bM + cells);
    uint8_t* bit = reinterpret_cast<uint8_t*>(lp + 2 * cells);
    guided_read<THREADS, CPT, CALC, TRAIN>(rd, a, bE, bM, lp, bit, s_rows, stride, s_exp, s_ctl + 1);
  }
}

// ---- guided band margins: one thread per path row ----
// grid ceil((read_hi - read_lo) / 256)
__global__ __launch_bounds__(256) void k_bmargin_guided_init(BandMargin bm) {
  const uint64_t i = (uint64_t)bm.read_lo + (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= bm.read_hi) return;
  bm.low[i] = GBM_NONE;
  bm.high[i] = GBM_NONE;
  bm.edge_rows[i] = 0u;
}

// grid (n_reads, ceil(max_T / 256)): thread j of block (r, c) owns lattice row c * 256 + j of read descs[r]
__global__ __launch_bounds__(256) void k_bmargin_guided(const ReadDesc* __restrict__ descs, const ReadState* __restrict__ st,
                                                        const uint32_t* __restrict__ pathn_all, const uint32_t* __restrict__ segrow_all,
                                                        const int32_t* __restrict__ guide, int bw, BandMargin bm) {
  const ReadDesc rd = descs[blockIdx.x];
  const int T = (int)rd.T, N = (int)rd.N;
  if ((int)(blockIdx.y * 256u) >= T || N < 2) return;
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
                               const int32_t* guide, int bw, const BandMargin& bm, hipStream_t s) {
  if (!bm.low || bm.read_lo >= bm.read_hi) return;
  hipLaunchKernelGGL(k_bmargin_guided_init, dim3((bm.read_hi - bm.read_lo + 255u) / 256u), dim3(256), 0, s, bm);
  if (n_reads <= 0 || max_T < 2) return;
  hipLaunchKernelGGL(k_bmargin_guided, dim3((unsigned)n_reads, (max_T + 255u) / 256u), dim3(256), 0, s, descs, st, tb.pathn,
                     tb.segrow, guide, bw, bm);
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

uint64_t guided_arena_bytes(uint64_t T, uint64_t bw, int job) {
  if (job == 0) return 0;
  const uint64_t cells = T * (2 * bw + 3);
  return (cells * (job == 2 ? 16 : 25) + 255) & ~255ull;  // bE, bM doubles; align: (float LPM, float LPE), one byte per decision
}

namespace {
// shapes, narrowest first: B = 2 bw + 3 <= THREADS * CPT
// groups: an UPPER BOUND on the workgroups launched per compute unit (what a CU can run beside each other at about 100 / 140 /
// 256 VGPRs per lane, the probability job's use with the product's flags). It only limits how many arenas a launch allocates:
// workgroups beyond what the hardware keeps resident wait their turn, fewer leave a CU partly idle. Nothing depends on it
// being exact, and it need not follow the compiler's register counts.
struct Shape { int threads, cpt, groups; };
constexpr Shape SHAPES[] = {{64, 1, 16}, {64, 4, 12}, {256, 16, 1}};
const Shape& shape_of(int bw) {
  const int B = 2 * bw + 3;
  for (const Shape& s : SHAPES)
    if (B <= s.threads * s.cpt) return s;
  return SHAPES[2];
}
size_t lds_bytes(int bw, int job) {  // the train job keeps the two forward rows only
  return (size_t)dynmath::STRICT_EXP_WORDS * 8 + (job == 2 ? 2 : 4) * (size_t)guided_row_stride(2 * bw + 3) * 8 + 16;
}
template <int THREADS, int CPT>
hipError_t launch_shape(int job, const GuidedArgs& a, int n_groups, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024) {  // (a wide window: the request exceeds the default dynamic-LDS limit)
    const void* fn = job == 2   ? reinterpret_cast<const void*>(&k_guided_reads<THREADS, CPT, false, true>)
                     : job == 1 ? reinterpret_cast<const void*>(&k_guided_reads<THREADS, CPT, true, false>)
                                : reinterpret_cast<const void*>(&k_guided_reads<THREADS, CPT, false, false>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  if (job == 2) hipLaunchKernelGGL((k_guided_reads<THREADS, CPT, false, true>), dim3(n_groups), dim3(THREADS), lds, s, a);
  else if (job == 1) hipLaunchKernelGGL((k_guided_reads<THREADS, CPT, true, false>), dim3(n_groups), dim3(THREADS), lds, s, a);
  else hipLaunchKernelGGL((k_guided_reads<THREADS, CPT, false, false>), dim3(n_groups), dim3(THREADS), lds, s, a);
  return hipGetLastError();
}
}  // namespace

// as many workgroups as a CU's 160 KiB of LDS and its registers hold beside each other
int guided_groups_per_cu(int bw, int job) {
  const int by_lds = (int)((150 * 1024) / lds_bytes(bw, job));
  const int by_waves = shape_of(bw).groups;
  return by_lds < 1 ? 1 : by_lds < by_waves ? by_lds : by_waves;
}

hipError_t launch_guided_reads(int job, const GuidedArgs& a, int n_groups, hipStream_t s) {
  if (a.n_reads <= 0 || n_groups <= 0) return hipSuccess;
  if (a.bw < 1 || a.bw > WIDE_MAX_HALF_BAND || job < 0 || job > 2) return hipErrorInvalidValue;
  if (job == 2 && !(a.tr.col_w && a.tr.col_s1 && a.tr.col_s2 && a.tr.trans)) return hipErrorInvalidValue;
  if (job != 0 && !a.arena) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(a.head, 0, 4, s)) return e;
  const size_t lds = lds_bytes(a.bw, job);
  const Shape& sh = shape_of(a.bw);
  if (sh.cpt == 1) return launch_shape<64, 1>(job, a, n_groups, lds, s);
  if (sh.threads == 64) return launch_shape<64, 4>(job, a, n_groups, lds, s);
  return launch_shape<256, 16>(job, a, n_groups, lds, s);
}

}  // namespace dynk
