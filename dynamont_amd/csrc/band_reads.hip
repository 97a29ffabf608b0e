// band_reads.hip -- the banded-lattice kernel: the reads the register sweeps of nt_kernels.hip do not take.
//
// The reference constructs with ANY band (src/cpp/aligner.cpp:21, aligner_bindings.cpp:191-199) and walks rows of
// 2 * bw + 3 band columns whatever bw is (NT_aligner_api.cpp:243-244). The tuned sweeps keep a lattice row in 64 lanes x 7
// registers: half bands up to 223, which covers every caller of the reference (band = 400, segment.py:45). Reads beyond that --
// a handle built with band > 447 AND more than 447 lattice columns -- and every read of a guided batch (dyn_batch_set_guide)
// take THIS kernel: the reference's algorithm in its own band-column addressing,
//   computeBounds          NT_aligner_api.cpp:90-108     cell (t, n) <-> band column c = n - start_t + 1, 1 <= c <= 2 bw + 1
//   backward               NT_aligner_api.cpp:158-207    stores bE and bM rows (16 B per cell)
//   forward + posterior    NT_aligner_api.cpp:110-152, 213-224   )
//   posterior-Viterbi      NT_aligner_api.cpp:338-363            )  one ascending sweep, previous rows in LDS
//   decision bit           NT_aligner_api.cpp:448                )
//   decodeMAP              NT_aligner_api.cpp:383-456    one lane walks the bits
//   runTraining            NT_aligner_api.cpp:462-561    per-column (w, s1, s2)
// One workgroup per read, thread i owns band columns i, i + THREADS, ...; a row is one pass + one barrier. The arithmetic is
// the reference's OWN, bit for bit, in every cell (dp_math_strict.hpp: the IEEE quotient, glibc's exp and fdlibm's log1p
// restated) -- no certificate, no table softplus: Z, the borders and the decision bits are the reference's whether or not the
// read carries a structural tie. It runs at a fraction of the tuned sweeps' rate (~25 B of HBM and ~300 instructions per
// cell); what it buys is that no band the reference accepts is refused, and that a window may follow a guide.
// Per-row outputs (pp, pathn, segrow, ReadState) are those of nt_kernels.hip's traceback: launch_segments / k_median / k_final
// follow unchanged.
//
// ONE body, band_read, for both windows of band_reads.hpp; a window is a policy, inlined, with no run-time branch per cell:
//   centre(t), bw      where a row's window lies and how wide it is
//   end_column         the band column the backward seed and Zf are read at
//   DIAGONAL           compile-time: the read's own B bounds the column loops (a launch holds reads of different B below the
//                      shape's THREADS x CPT), and the train job keeps per-thread running sums (below)
//   boundaries         forward / Viterbi seed and Zb at (0, 0) = band column bw + 1 of row 0 (centre(0) = 0 in both); a cell
//                      outside its row's window is -inf, and a read whose windows do not connect then fails the reference's
//                      own Z check (DYN_READ_Z_MISMATCH): an infeasible guide costs that read only
//   geometry           guided: THREADS x CPT shapes picked per launch from B = 2 bw + 3, the four LDS rows sized from B (dynamic
//                      LDS, every carve a multiple of 16 B), the per-thread row registers by CPT; shapes of CPT <= 4 are fully
//                      unrolled (registers, no scratch), several workgroups share a CU. Diagonal: <256, 16> (a wide read has
//                      B >= 451), static LDS rows of WIDE_MAX_B doubles, one workgroup per CU
//   Z only             nothing of the lattice is stored: the backward rows live in LDS, no arena
//   train              the backward sweep stores bE / bM (16 B per cell, nothing else in the arena); the forward sweep forms
//                      LPM / LPE as the align job does and, instead of posterior-Viterbi and the traceback, adds
//                      g = exp(LPM) + exp(LPE) into the read's per-column sums (w, s1, s2) of TrainBuffers.
//                      Guided: a per-row read-modify-write of the column sums in global memory -- the lanes of a row own
//                      distinct lattice columns and the row's barrier separates it from the next row, whose owner of a column
//                      may be another lane after a shift of any size. Nothing is held across rows: every access is entry n - 1
//                      of a cell's own column n in [1, N). Two LDS rows (the forward rows) only.
//                      Diagonal: the shift is 0 or 1, so a thread's band column covers ONE lattice column until the band moves;
//                      it keeps running sums in registers and flushes them when it does. The two schemes group a column's
//                      additions differently -- their sums agree to rounding, not bit for bit -- so neither replaces the other
//                      silently.
//                      Either way a column's sum is formed in ascending t, without atomics: the same bits whichever workgroup
//                      takes the read.
// A diagonal guide at bw = min(band / 2, N / 2) is the reference's band: the results are the diagonal window's bit for bit.
// A third policy, LiveGuideWindow, is GuideWindow for the launch that refines every read's guide inside the launch (k_band_reads
// with REFINE, below): the same window, read through a pointer the kernel may write behind.
#include "band_reads.hpp"

#include "border_kernels.hpp"
#include "interval_kernels.hpp"
#include "soft_level_kernels.hpp"
#include "sample_kernels.hpp"
#include "dp_math_strict.hpp"

#include <utility>

namespace dynk {

using dynmath::NEG_INF;

namespace {
__host__ __device__ constexpr int guided_row_stride(int B) { return (B + 1) & ~1; }  // doubles per LDS row: rows stay 16 B aligned
}

// the two windows (named in dynk, not in the unnamed namespace: the kernels' symbols then read k_band_reads<GuideWindow, ..>)
struct GuideWindow {
  static constexpr bool DIAGONAL = false;
  const int32_t* __restrict__ gd;  // centre(t) = gd[t - 1], t >= 1
  int bw;
  __device__ __forceinline__ GuideWindow(const ReadDesc& rd, const BandArgs& a) : gd(a.guide + rd.sig_off), bw(a.bw) {}
  __device__ __forceinline__ int centre(int t) const { return t > 0 ? (int)gd[t - 1] : 0; }
  // band column of (T-1, N-1) in a row that starts at start_last; outside 1 .. 2 bw + 1: no seed, Zf = -inf
  __device__ __forceinline__ int end_column(int start_last, int N) const { return (N - 1) - start_last + 1; }
  static __device__ __forceinline__ int row_stride(const BandArgs& a) { return guided_row_stride(2 * a.bw + 3); }
  static __device__ __forceinline__ char* lds(char* dynamic) { return dynamic; }  // sized per launch: lds_bytes below
};

// GuideWindow for the launch that refines every read's guide itself (BandArgs::refine_rounds > 1): the workgroup REWRITES the
// guide between two alignments of a read, so the pointer is neither const nor __restrict__, and a centre is fetched by a relaxed
// atomic load at workgroup scope -- a vector load the compiler neither hoists across the rewrite nor turns into a scalar load
// (the scalar data cache is not updated by the kernel's own vector stores: a second alignment could run inside the old guide)
struct LiveGuideWindow {
  static constexpr bool DIAGONAL = false;
  int32_t* gd;
  int bw;
  __device__ __forceinline__ LiveGuideWindow(const ReadDesc& rd, const BandArgs& a) : gd(a.guide + rd.sig_off), bw(a.bw) {}
  __device__ __forceinline__ int centre(int t) const {
    return t > 0 ? (int)__hip_atomic_load(gd + (t - 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
  }
  __device__ __forceinline__ int end_column(int start_last, int N) const { return (N - 1) - start_last + 1; }
  static __device__ __forceinline__ int row_stride(const BandArgs& a) { return guided_row_stride(2 * a.bw + 3); }
  static __device__ __forceinline__ char* lds(char* dynamic) { return dynamic; }
};

struct DiagonalWindow {
  static constexpr bool DIAGONAL = true;
  double ratio;
  int bw;
  __device__ __forceinline__ DiagonalWindow(const ReadDesc& rd, const BandArgs&) : ratio(rd.ratio), bw((int)rd.bw) {}
  __device__ __forceinline__ int centre(int t) const { return diagonal_centre(t, ratio); }
  __device__ __forceinline__ int end_column(int, int) const { return bw + 1; }  // E[(T-1) * B + bw + 1] (:170), forwardE[T * B - bw - 2] (:285)
  static __device__ __forceinline__ int row_stride(const BandArgs&) { return WIDE_MAX_B; }
  // four rows of WIDE_MAX_B doubles whatever the job and the reads' B, declared statically: the launch asks for no dynamic LDS
  // and raises no limit. More than half a CU's LDS, so the dispatcher never puts two of the launch's workgroups (at most one
  // per CU) on one CU while another stays empty
  static __device__ __forceinline__ char* lds(char*) {
    __shared__ __attribute__((aligned(16))) char s_lds[dynmath::STRICT_EXP_WORDS * 8 + 4 * WIDE_MAX_B * 8 + 16];
    return s_lds;
  }
};

namespace {

// one read; lds: [STRICT_EXP_WORDS u64 | 4 rows (guided TRAIN: 2) of `stride` doubles | 4 ints]
// TRAIN: the statistics pass instead of posterior-Viterbi + traceback. CALC: align(calc_probabilities = true).
template <class Window, int THREADS, int CPT, bool CALC, bool TRAIN>
__device__ void band_read(const ReadDesc& rd, const BandArgs& a, double* __restrict__ bE, double* __restrict__ bM,
                          float* __restrict__ lp, uint8_t* __restrict__ bit, double* s_rows, int stride, const uint64_t* s_exp,
                          int* s_bad) {
  constexpr int UNROLL = CPT <= 4 ? CPT : 1;
  constexpr bool SUMS = TRAIN && Window::DIAGONAL;  // the train job's per-thread running sums
  const Window win(rd, a);
  const int tid = threadIdx.x;
  const int T = (int)rd.T, N = (int)rd.N, bw = win.bw, B = 2 * bw + 3;
  const double m1 = a.m1, e2 = a.e2;
  const double* __restrict__ sg = a.sig + rd.sig_off;
  const Emis* __restrict__ pr = a.par + rd.par_off;        // entry n - 1 <-> lattice column n
  double* nxE = s_rows;               // backward: row t + 1;  forward: fE of row t - 1
  double* nxM = s_rows + stride;      //                         forward: fM of row t - 1
  double* pvE = TRAIN ? nullptr : s_rows + 2 * stride;  // forward: vE of row t - 1 (TRAIN: no such rows in LDS)
  double* pvM = TRAIN ? nullptr : s_rows + 3 * stride;  // forward: vM of row t - 1
  if (tid == 0) *s_bad = 0;
  auto at = [&](const double* row, int c) { return (c >= 0 && c < B) ? row[c] : NEG_INF; };  // guard columns and beyond: -inf (:129-130)
  auto centre = [&](int t) { return win.centre(t); };
  // this thread has a k-th band column: under the diagonal window the walk ends at the read's own B (<= THREADS * CPT: the host
  // refuses half bands above WIDE_MAX_HALF_BAND); a guided launch picked the shape from its B and walks all CPT
  auto more = [&](int k) { return Window::DIAGONAL ? tid + k * THREADS < B : k < CPT; };

  // ---- backward (NT_aligner_api.cpp:158-207): t = T-2 .. 0 ----
  {
    const int c_seed = win.end_column(centre(T - 1) - bw, N);
#pragma unroll UNROLL
    for (int k = 0; more(k); ++k) {
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
    const int shift = start_next - start;  // start_{t+1} - start_t >= 0 (:177-184)
    start_next = start;
    const double x = sg[t];
    bad |= !(__builtin_fabs(x) <= 1.7976931348623157e308);
    double oE[CPT], oM[CPT];
#pragma unroll UNROLL
    for (int k = 0; more(k); ++k) {
      const int c = tid + k * THREADS;
      double ext = NEG_INF, bm = NEG_INF;
      if (c < B) {
        const int n = start + c - 1;
        if (c >= 1 && c <= 2 * bw + 1 && n >= n_lo && n < n_hi) {
          const int cn = c - shift;  // band column of lattice column n in row t + 1
          if (n + 1 < N) ext = (at(nxM, cn + 1) + dynmath::log_normal_pdf_strict(x, pr[n])) + m1;  // :192-195
          if (n > 0) {
            const double score = dynmath::log_normal_pdf_strict(x, pr[n - 1]);
            const double e_next = at(nxE, cn);
            bm = e_next + score;                                                            // :200
            ext = dynmath::log_plus_strict(ext, (e_next + score) + e2, s_exp);               // :201
          }
        }
      }
      oE[k] = ext;
      oM[k] = bm;
    }
    __syncthreads();
#pragma unroll UNROLL
    for (int k = 0; more(k); ++k) {
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
  const double Zb_raw = nxE[bw + 1];  // (0, 0): start_0 = -bw; backwardE[bw + 1] (:286)
  __syncthreads();
  const double Zb = *s_bad ? NEG_INF : Zb_raw;  // an infinite / NaN sample: "alignment scores do not match", as the tuned sweeps report it

  // ---- forward (:110-152) + posterior (:213-224) + posterior-Viterbi (:338-363) + decision bit (:448), t = 1 .. T-1 ----
#pragma unroll UNROLL
  for (int k = 0; more(k); ++k) {
    const int c = tid + k * THREADS;
    if (c < B) {
      const double v = (c == bw + 1) ? 0.0 : NEG_INF;  // (0, 0): E[bw + 1] = 0 (:120, :336)
      nxE[c] = v;
      nxM[c] = NEG_INF;
      if (!TRAIN) {
        pvE[c] = v;
        pvM[c] = NEG_INF;
      }
    }
  }
  // TRAIN: the read's column sums start at 0 (entry n - 1 <-> lattice column n, N - 1 entries). Not __restrict__: a column's
  // word is written by one lane and read by another in a later row
  double* cw = TRAIN ? a.tr.col_w + rd.par_off : nullptr;
  double* cs1 = TRAIN ? a.tr.col_s1 + rd.par_off : nullptr;
  double* cs2 = TRAIN ? a.tr.col_s2 + rd.par_off : nullptr;
  if (TRAIN) {
    for (int n = tid; n < N - 1; n += THREADS) cw[n] = cs1[n] = cs2[n] = 0.0;
  }
  // SUMS: this thread's running sums for the lattice column its k-th band column currently covers (otherwise unused: the arrays
  // and flush, never called, compile to nothing)
  double aw[CPT], a1[CPT], a2[CPT];
  auto flush = [&](int start_old, bool clear) {  // band column c covered lattice column start_old + c - 1 until now
#pragma unroll 1
    for (int k = 0; more(k); ++k) {
      const int n_old = start_old + tid + k * THREADS - 1;
      if (n_old >= 1 && n_old < N && aw[k] != 0.0) {
        cw[n_old - 1] += aw[k];
        cs1[n_old - 1] += a1[k];
        cs2[n_old - 1] += a2[k];
      }
      if (clear) aw[k] = a1[k] = a2[k] = 0.0;
    }
  };
  if constexpr (SUMS) {
#pragma unroll 1
    for (int k = 0; k < CPT; ++k) aw[k] = a1[k] = a2[k] = 0.0;
  }
  __syncthreads();
  int start_prev = -bw;
  for (int t = 1; t < T; ++t) {
    const int mid = centre(t), start = mid - bw;
    const int n_lo = start > 1 ? start : 1, n_hi = (mid + bw + 1 < N) ? mid + bw + 1 : N;  // forward never fills n = 0 (:126-127)
    const int shift = start - start_prev;  // >= 0 (:131-138)
    if constexpr (SUMS) {
      if (shift) {  // the band moves up by one column
        flush(start_prev, true);
        __syncthreads();  // the next owner of a column adds to the same words later
      }
    }
    start_prev = start;
    const double x = sg[t - 1];
    double ofE[CPT], ofM[CPT], ovE[CALC ? CPT : 1], ovM[CALC ? CPT : 1];
#pragma unroll UNROLL
    for (int k = 0; more(k); ++k) {
      const int c = tid + k * THREADS;
      double fM = NEG_INF, fE = NEG_INF, vM = NEG_INF, vE = NEG_INF;
      if (c < B) {
        const int n = start + c - 1;
        if (c >= 1 && c <= 2 * bw + 1 && n >= n_lo && n < n_hi) {
          const int cp = c + shift;  // band column of lattice column n in row t - 1
          const double score = dynmath::log_normal_pdf_strict(x, pr[n - 1]);               // :144
          fM = (at(nxE, cp - 1) + score) + m1;                                              // :146
          fE = dynmath::log_plus_strict((at(nxM, cp) + score) + 0.0, (at(nxE, cp) + score) + e2, s_exp);  // :147-149, e1 = log 1
          if (TRAIN) {
            const size_t cell = (size_t)t * B + c;
            const double LPM = (fM + bM[cell]) - Zb, LPE = (fE + bE[cell]) - Zb;            // :222
            const double g = exp(LPM) + exp(LPE);                                           // :505-512
            if constexpr (SUMS) {
              aw[k] += g;
              a1[k] += g * x;
              a2[k] += (g * x) * x;
            } else {
              // n in [max(start, 1), min(centre + bw + 1, N)): entry n - 1 lies in the read's N - 1 entries whatever the shift.
              // This lane alone owns column n in this row; the barrier below orders it against the next row's owner.
              cw[n - 1] += g;
              cs1[n - 1] += g * x;
              cs2[n - 1] += (g * x) * x;
            }
          } else if (CALC) {
            const size_t cell = (size_t)t * B + c;
            const double LPM = (fM + bM[cell]) - Zb, LPE = (fE + bE[cell]) - Zb;            // :222
            vM = at(pvE, cp - 1) + LPM;                                                     // :360
            const double um = at(pvM, cp), ue = at(pvE, cp);
            vE = (um < ue ? ue : um) + LPE;                                                 // :361 (std::max)
            lp[2 * cell] = (float)LPM;
            lp[2 * cell + 1] = (float)LPE;
            bit[cell] = (vE == um + LPE) ? 1 : 0;                                           // :448
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
    for (int k = 0; more(k); ++k) {
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
  if constexpr (SUMS) flush(start_prev, false);
  const int c_last = win.end_column(start_prev, N);  // (T = 1: row 0)
  const double Zf = (c_last >= 1 && c_last <= 2 * bw + 1) ? nxE[c_last] : NEG_INF;
  // Z check (:285-291 / :619-625)
  const double size = (double)((uint64_t)T * (uint64_t)B);
  const bool ok = !(isinf(Zf) || isinf(Zb)) && !(__builtin_fabs(Zf - Zb) / size > 1e-8);
  int status = ok ? 0 : a.z_fail_status;
  uint32_t n_seg = 0;
  __syncthreads();

  // ---- decodeMAP (:383-456): one lane walks the decision bits from (T-1, N-1) in state E ----
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
    // expected transition counts (:641-725): every path makes N - 1 moves and T - 1 - 2 (N - 1) extensions
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

// one workgroup takes reads off a queue until it is empty; its lattice arena (jobs 1 and 2) holds one read at a time.
// PHASES: the lattice phases (lattice_phase.hpp) behind every read, diagonal window and align with probabilities only. The
// read's lattice is still in the arena when band_read returns (its closing barrier has made the lattice, the state and the
// segrow that thread 0 wrote visible to the workgroup), and the barrier at the head of the loop keeps the arena until every
// thread is done with it. Border confidence: all threads; posterior samples: the first wave, a lane per sample; credible
// intervals and soft levels: a thread per column walks that column's row interval.
// REFINE (LiveGuideWindow, align with probabilities): the workgroup that holds a read refines its guide, behind every band_read
// what k_guide_refine (guided_band.hip) does for the read between two launches of the round scheme, rule for rule: the
// alignment is counted; a failed read is finished; the called path g'[s] = pathn[s + 1] (0 before the first border) is compared
// with the guide; equal everywhere: converged; otherwise, unless this was alignment refine_rounds, g' becomes the guide and the
// read is aligned again in the same arena. Only then does the workgroup take the next read: a launch lasts as long as its
// reads' alignments, not as refine_rounds times its longest read. With BandArgs::active the launch takes the listed descriptors
// only (the guide rescue); a self-guided ticket passes none.
template <class Window, int THREADS, int CPT, bool CALC, bool TRAIN, int PHASES, bool REFINE = false>
__global__ __launch_bounds__(THREADS) void k_band_reads(const BandArgs a) {
  static_assert(PHASES == 0 || (Window::DIAGONAL && CALC && !TRAIN && !REFINE), "lattice phases: diagonal window, align with probabilities");
  static_assert((PHASES & ~LATTICE_PHASE_BITS) == 0 && (!(PHASES & (JOB_INTERVAL | JOB_SOFT)) || PHASES == JOB_INTERVAL || PHASES == JOB_SOFT),
                "the credible intervals and the soft levels run alone");
  extern __shared__ __attribute__((aligned(16))) char g_lds[];
  char* lds = Window::lds(g_lds);
  const int stride = Window::row_stride(a);
  uint64_t* s_exp = reinterpret_cast<uint64_t*>(lds);
  double* s_rows = reinterpret_cast<double*>(lds + dynmath::STRICT_EXP_WORDS * 8);
  int* s_ctl = reinterpret_cast<int*>(s_rows + (TRAIN && !Window::DIAGONAL ? 2 : 4) * stride);  // [0] next read, [1] s_bad, [2] REFINE: the path differs from the guide
  for (int i = threadIdx.x; i < dynmath::STRICT_EXP_WORDS; i += THREADS) s_exp[i] = a.exp_tab[i];
  char* arena = a.arena + (size_t)blockIdx.x * a.arena_bytes;
  for (;;) {
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[0] = (int)atomicAdd(a.head, 1u);
    __syncthreads();
    const int k = s_ctl[0];
    // a refinement round (launch_guide_refine) or the guide rescue (launch_rescue_select) hands over the list of the reads to
    // align and its length on the device; an empty list ends the workgroup at this first queue read
    // LISTS: launch_band_reads refuses a list beside the samples, the intervals and the soft levels, and those kernels hold no
    // branch for it
    constexpr bool LISTS = (PHASES & (JOB_SAMPLE | JOB_INTERVAL | JOB_SOFT)) == 0;
    const bool listed = LISTS && a.active != nullptr;
    if (k >= (listed ? (int)*a.n_active : a.n_reads)) break;
    const ReadDesc rd = LISTS ? a.descs[listed ? a.active[k] : (uint32_t)k] : a.descs[k];
    const size_t cells = (size_t)rd.T * (size_t)(2 * Window(rd, a).bw + 3);
    double* bE = reinterpret_cast<double*>(arena);
    double* bM = bE + cells;
    float* lp = reinterpret_cast<float*>(bM + cells);
    uint8_t* bit = reinterpret_cast<uint8_t*>(lp + 2 * cells);
    if constexpr (REFINE) {
      const int T = (int)rd.T;
      int32_t* gd = a.guide + rd.sig_off;
      const uint32_t* pathn = a.tb.pathn + rd.path_off;  // written by thread 0 in this launch: neither const data nor __restrict__
      uint32_t round = 1;
      for (;; ++round) {
        // cleared in front of the alignment: its barriers order this against the comparison below, and the barrier behind the
        // rewrite against the last look at the word
        if (threadIdx.x == 0) s_ctl[2] = 0;
        band_read<Window, THREADS, CPT, CALC, TRAIN>(rd, a, bE, bM, lp, bit, s_rows, stride, s_exp, s_ctl + 1);
        // behind band_read's closing barrier: the state, pathn and segrow of thread 0 are visible to the workgroup
        if (__hip_atomic_load(&a.st[rd.read].status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0) break;  // failed: that is its result
        const int first = rd.N >= 2 ? (int)__hip_atomic_load(a.tb.segrow + rd.seg_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : T;
        int differs = 0;
        for (int s = (int)threadIdx.x; s < T - 1; s += THREADS) {
          const int32_t g = s + 1 >= first ? (int32_t)(pathn[s + 1] & 0x7fffffffu) : 0;
          differs |= g != gd[s];
        }
        if (differs) s_ctl[2] = 1;
        __syncthreads();
        if (!s_ctl[2]) {
          if (threadIdx.x == 0) a.converged[rd.read] = 1u;
          break;
        }
        if (round == (uint32_t)a.refine_rounds) break;  // the guide stays the one the last alignment used
        for (int s = (int)threadIdx.x; s < T - 1; s += THREADS) gd[s] = s + 1 >= first ? (int32_t)(pathn[s + 1] & 0x7fffffffu) : 0;
        __syncthreads();  // the whole guide is rewritten before the next alignment reads a centre
      }
      if (threadIdx.x == 0) a.rounds[rd.read] = round;  // alignments run (the launch cleared the counts)
    } else {
      band_read<Window, THREADS, CPT, CALC, TRAIN>(rd, a, bE, bM, lp, bit, s_rows, stride, s_exp, s_ctl + 1);
    }
    if constexpr (PHASES != 0) {
      if (__hip_atomic_load(&a.st[rd.read].status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0) {
        const BorderBand band{(int)rd.T, (int)rd.N, (int)rd.bw, rd.ratio};
        const BorderCellWide lpm{band, lp};
        [[maybe_unused]] const SampleLpeWide lpe{band, lp};
        const int tid = (int)threadIdx.x;
        if constexpr ((PHASES & JOB_BORDER) != 0) border_confidence_read(lpm, rd, a.tb.segrow, a.border_p, a.border_window_p, a.border_window, tid, THREADS);
        if constexpr ((PHASES & JOB_SAMPLE) != 0)
          if (tid < 64) posterior_samples_read(lpm, lpe, rd, a.sample, tid);
        if constexpr ((PHASES & JOB_INTERVAL) != 0) border_interval_read_columns(lpm, band, rd, a.tb.segrow, a.interval, tid, THREADS);
        if constexpr ((PHASES & JOB_SOFT) != 0) soft_levels_read_columns(lpm, lpe, band, rd, a.sig + rd.sig_off, a.soft, tid, THREADS);
      }
    }
  }
}

uint64_t band_arena_bytes(uint64_t T, uint64_t bw, int job) {
  if (job == 0) return 0;
  const uint64_t cells = T * (2 * bw + 3);
  return (cells * (job == 2 ? 16 : 25) + 255) & ~255ull;  // bE, bM doubles; align: (float LPM, float LPE), one byte per decision
}

namespace {
// guided shapes, narrowest first: B = 2 bw + 3 <= THREADS * CPT
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

template <class Window, int THREADS, int CPT, bool CALC, bool TRAIN, int PHASES = 0, bool REFINE = false>
hipError_t launch_kernel(const BandArgs& a, int n_groups, size_t lds, hipStream_t s) {
  if (lds > 48 * 1024) {  // (a wide guided window: the request exceeds the default dynamic-LDS limit; diagonal launches ask for none)
    const void* fn = reinterpret_cast<const void*>(&k_band_reads<Window, THREADS, CPT, CALC, TRAIN, PHASES, REFINE>);
    if (const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)) return e;
  }
  hipLaunchKernelGGL((k_band_reads<Window, THREADS, CPT, CALC, TRAIN, PHASES, REFINE>), dim3(n_groups), dim3(THREADS), lds, s, a);
  return hipGetLastError();
}
template <class Window, int THREADS, int CPT>
hipError_t launch_shape(int job, const BandArgs& a, int n_groups, size_t lds, hipStream_t s) {
  if (job == 2) return launch_kernel<Window, THREADS, CPT, false, true>(a, n_groups, lds, s);
  if (job == 1) return launch_kernel<Window, THREADS, CPT, true, false>(a, n_groups, lds, s);
  return launch_kernel<Window, THREADS, CPT, false, false>(a, n_groups, lds, s);
}
// the diagonal launch of align with probabilities: one kernel for every set of lattice phases on lattice_phase.hpp's list
template <size_t... I>
hipError_t launch_diagonal_phases(int phases, const BandArgs& a, int n_groups, hipStream_t s, std::index_sequence<I...>) {
  hipError_t e = hipErrorInvalidValue;
  ((phases == LATTICE_PHASE_SETS[I] ? void(e = launch_kernel<DiagonalWindow, 256, 16, true, false, LATTICE_PHASE_SETS[I]>(a, n_groups, 0, s)) : void()), ...);
  return e;
}
}  // namespace

// guided: as many workgroups as a CU's 160 KiB of LDS and its registers hold beside each other
int band_groups_per_cu(bool guided, int bw, int job) {
  if (!guided) return 1;
  const int by_lds = (int)((150 * 1024) / lds_bytes(bw, job));
  const int by_waves = shape_of(bw).groups;
  return by_lds < 1 ? 1 : by_lds < by_waves ? by_lds : by_waves;
}

hipError_t launch_band_reads(int job, const BandArgs& a, int n_groups, hipStream_t s) {
  if (a.n_reads <= 0 || n_groups <= 0) return hipSuccess;
  if (job < 0 || job > 2 || (a.guide && (a.bw < 1 || a.bw > WIDE_MAX_HALF_BAND))) return hipErrorInvalidValue;
  if (job == 2 && !(a.tr.col_w && a.tr.col_s1 && a.tr.col_s2 && a.tr.trans)) return hipErrorInvalidValue;
  if (job != 0 && !a.arena) return hipErrorInvalidValue;
  if (a.border_window > 0 && (a.guide || job != 1 || !a.border_p || !a.border_window_p)) return hipErrorInvalidValue;
  const int phases = lattice_phases(job == 1, a.sample.count, a.interval.tail, a.border_window);
  const bool soft = phases == JOB_SOFT;  // dyn_aligner_set_soft_levels
  if (soft && (a.guide || a.active || a.border_window > 0 || !a.soft.weight || a.soft.zero != 0)) return hipErrorInvalidValue;
  if (!soft && job == 1 && a.sample.count != 0 && (a.sample.count < 0 || a.guide || a.active || job != 1 || a.sample.count > PS_MAX_SAMPLES || !a.sample.start))
    return hipErrorInvalidValue;
  const bool interval = phases == JOB_INTERVAL;  // dyn_aligner_set_border_interval
  if (interval && (a.guide || a.active || a.border_window > 0 || !a.interval.mean || !(a.interval.tail < 0.5))) return hipErrorInvalidValue;
  const bool refine = a.refine_rounds > 1;  // every read refined inside this launch
  if (refine && (!a.guide || job != 1 || a.border_window > 0 || !a.rounds || !a.converged)) return hipErrorInvalidValue;
  if (const hipError_t e = hipMemsetAsync(a.head, 0, 4, s)) return e;
  if (!a.guide) {
    // (static LDS, as every diagonal launch)
    if (job == 1) return launch_diagonal_phases(phases, a, n_groups, s, std::make_index_sequence<N_LATTICE_PHASE_SETS>{});
    return launch_shape<DiagonalWindow, 256, 16>(job, a, n_groups, 0, s);
  }
  const size_t lds = lds_bytes(a.bw, job);
  const Shape& sh = shape_of(a.bw);
  if (refine) {
    if (sh.cpt == 1) return launch_kernel<LiveGuideWindow, 64, 1, true, false, 0, true>(a, n_groups, lds, s);
    if (sh.threads == 64) return launch_kernel<LiveGuideWindow, 64, 4, true, false, 0, true>(a, n_groups, lds, s);
    return launch_kernel<LiveGuideWindow, 256, 16, true, false, 0, true>(a, n_groups, lds, s);
  }
  if (sh.cpt == 1) return launch_shape<GuideWindow, 64, 1>(job, a, n_groups, lds, s);
  if (sh.threads == 64) return launch_shape<GuideWindow, 64, 4>(job, a, n_groups, lds, s);
  return launch_shape<GuideWindow, 256, 16>(job, a, n_groups, lds, s);
}

}  // namespace dynk
