// cell_math.hip -- test-only translation unit (tests/test_gpu_cell_math.py): every piece of the per-cell arithmetic of
// dp_math.hpp, dp_math_strict.hpp and dp_cell.hpp run ON THE DEVICE on arrays of arguments, one function at a time, so that
// the bits the GPU computes can be laid beside the bits the g++ build of the same headers computes.
//
// Compiled by the test with the product's hipcc flags (dynamont_amd/_native.py, hipcc_flags()) into a shared library and
// loaded with ctypes. Launch geometry is the sweeps': 256-thread groups of four whole 64-lane waves, CPL = 7 cells per lane
// (lane l of a wave holds the cells 7 l .. 7 l + 6 of the wave's 448), every lane live -- log_plus_finish_certified ballots
// over the wave. The three tables are built by the host functions dynamont_mi.cpp uploads them with, in its layout (softplus
// nodes, 2^(i/128), glibc's exp table), and staged into LDS by the loop k_read_queue stages them with; LDS = false leaves
// them in global memory.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "dp_cell.hpp"

using namespace dynmath;
using dynk::CPL;
using dynk::Emis;
using dynk::P;

namespace {

constexpr int TAB_NODES = SP_NODES + EXP128_NODES + STRICT_EXP_WORDS / 2;
constexpr int MAX_IO = 6;

enum Op {
  OP_EXP_STRICT = 0,     // in: x                        out: exp_strict_vec
  OP_LOG1P_STRICT = 1,   // in: e                        out: log1p_strict_vec
  OP_LOG_PLUS_STRICT = 2,  // in: x, y                   out: log_plus_strict_vec, log_plus_strict_from(L.hi, L.diff)
  OP_PDF_STRICT = 3,     // in: x, mean, sd, 1/sd, -log sd   out: pdf strict (division), cert, cert4 (emission_vec<ARITH_STRICT>),
                         //                                       div_by_const, div_by_const4, (x - mean) / sd
  OP_LOG_PLUS = 4,       // in: x, y                     out: log_plus_issue + log_plus_finish, ... + log_plus_finish3
  OP_SOFTPLUS = 5,       // in: d                        out: softplus_table_vec, softplus_table3_vec
  OP_PDF = 6,            // in: x, mean, 1/sd, -log sd   out: emission_vec<ARITH_DEFAULT> (log_normal_pdf_vec)
  OP_EXP128 = 7,         // in: x                        out: exp_table128_vec, min_hw(., 1.0)
  OP_EMIS_FOLDED = 8,    // in: x, mean, 1/sd, -log sd   out: set_emis<ARITH_FOLDED> + emission_vec<ARITH_FOLDED>
  OP_LOG_PLUS_CERT = 9,  // in: x, y                     out: log_plus_issue + log_plus_finish_certified; fb[wave] = fallbacks
  N_OPS = 10
};

struct Args {
  const double* in[MAX_IO];
  double* out[MAX_IO];
  uint32_t* fb;
  long n_waves;
};

__device__ __forceinline__ void load7(const double* __restrict__ src, long base, double (&v)[CPL]) {
#pragma unroll
  for (int j = 0; j < CPL; ++j) v[j] = src[base + j];
}
__device__ __forceinline__ void store7(double* __restrict__ dst, long base, const double (&v)[CPL]) {
#pragma unroll
  for (int j = 0; j < CPL; ++j) dst[base + j] = v[j];
}

template <int OP>
__device__ __forceinline__ void cell_op(const Args& a, long base, long wave, const SoftplusNode* s_tab) {
  double x[CPL], y[CPL], o[CPL], o2[CPL];
  if constexpr (OP == OP_EXP_STRICT) {
    load7(a.in[0], base, x);
    exp_strict_vec<CPL>(x, o, dynk::strict_tab(s_tab));
    store7(a.out[0], base, o);
  } else if constexpr (OP == OP_LOG1P_STRICT) {
    load7(a.in[0], base, x);
    log1p_strict_vec<CPL>(x, o);
    store7(a.out[0], base, o);
  } else if constexpr (OP == OP_LOG_PLUS_STRICT) {
    load7(a.in[0], base, x);
    load7(a.in[1], base, y);
    log_plus_strict_vec<CPL>(x, y, o, dynk::strict_tab(s_tab));
    store7(a.out[0], base, o);
    SoftplusLookup<CPL> L;  // the fallback's operands as the sweeps hand them over: hi and diff of the issued lookup
    log_plus_issue<CPL>(x, y, L, s_tab);
#pragma unroll
    for (int j = 0; j < CPL; ++j) o2[j] = log_plus_strict_from(L.hi[j], L.diff[j], dynk::strict_tab(s_tab));
    store7(a.out[1], base, o2);
  } else if constexpr (OP == OP_PDF_STRICT) {
    double mean[CPL], sd[CPL], inv[CPL], nls[CPL], ylo[CPL], os[CPL], oc[CPL], oc4[CPL], q5[CPL], q4[CPL], q[CPL];
    load7(a.in[0], base, x);
    load7(a.in[1], base, mean);
    load7(a.in[2], base, sd);
    load7(a.in[3], base, inv);
    load7(a.in[4], base, nls);
    EmisV<CPL> p;
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      const Emis e{mean[j], inv[j], nls[j], sd[j]};
      dynk::set_emis<dynk::ARITH_STRICT>(p, j, e);
      ylo[j] = recip_lo(sd[j], inv[j]);  // on the device, as the sweeps form it at every hand-over
      os[j] = log_normal_pdf_strict(x[j], e);
      const double d = x[j] - mean[j];
      q5[j] = div_by_const(d, sd[j], inv[j]);
      q4[j] = div_by_const4(d, sd[j], inv[j], ylo[j]);
      q[j] = d / sd[j];
    }
    // the sweeps evaluate ONE sample against the seven cells of a lane; here every cell has a sample of its own
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      log_normal_pdf_cert_vec<CPL>(x[j], p, sd, o);
      oc[j] = o[j];
      dynk::emission_vec<dynk::ARITH_STRICT>(x[j], p, sd, ylo, o);
      oc4[j] = o[j];
    }
    store7(a.out[0], base, os);
    store7(a.out[1], base, oc);
    store7(a.out[2], base, oc4);
    store7(a.out[3], base, q5);
    store7(a.out[4], base, q4);
    store7(a.out[5], base, q);
  } else if constexpr (OP == OP_LOG_PLUS) {
    load7(a.in[0], base, x);
    load7(a.in[1], base, y);
    SoftplusLookup<CPL> L;
    log_plus_issue<CPL>(x, y, L, s_tab);
    log_plus_finish<CPL>(L, o);
    log_plus_finish3<CPL>(L, o2);
    store7(a.out[0], base, o);
    store7(a.out[1], base, o2);
  } else if constexpr (OP == OP_SOFTPLUS) {
    load7(a.in[0], base, x);
    softplus_table_vec<CPL>(x, o, s_tab);
    softplus_table3_vec<CPL>(x, o2, s_tab);
    store7(a.out[0], base, o);
    store7(a.out[1], base, o2);
  } else if constexpr (OP == OP_PDF || OP == OP_EMIS_FOLDED) {
    constexpr int ARITH = OP == OP_PDF ? dynk::ARITH_DEFAULT : dynk::ARITH_FOLDED;
    double mean[CPL], inv[CPL], nls[CPL];
    const double none[1] = {0.0};
    load7(a.in[0], base, x);
    load7(a.in[1], base, mean);
    load7(a.in[2], base, inv);
    load7(a.in[3], base, nls);
    EmisV<CPL> p;
#pragma unroll
    for (int j = 0; j < CPL; ++j) dynk::set_emis<ARITH>(p, j, Emis{mean[j], inv[j], nls[j], 0.0});
#pragma unroll
    for (int j = 0; j < CPL; ++j) {
      dynk::emission_vec<ARITH>(x[j], p, none, none, o);
      o2[j] = o[j];
    }
    store7(a.out[0], base, o2);
  } else if constexpr (OP == OP_EXP128) {
    load7(a.in[0], base, x);
    exp_table128_vec<CPL>(x, o, dynk::exp128_tab(s_tab));
    const double one = 1.0;
#pragma unroll
    for (int j = 0; j < CPL; ++j) o2[j] = min_hw(o[j], one);  // forward_train_chain: a stay probability is <= 1
    store7(a.out[0], base, o);
    store7(a.out[1], base, o2);
  } else if constexpr (OP == OP_LOG_PLUS_CERT) {
    load7(a.in[0], base, x);
    load7(a.in[1], base, y);
    SoftplusLookup<CPL> L;
    uint32_t nfb = 0;
    log_plus_issue<CPL>(x, y, L, s_tab);
    dynk::log_plus_finish_certified(L, o, dynk::strict_tab(s_tab), nfb);
    store7(a.out[0], base, o);
    if ((threadIdx.x & 63) == 0) a.fb[wave] = nfb;  // wave-uniform
  }
}

template <int OP, bool LDS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_cell(const Args a,
                                                                                        const SoftplusNode* __restrict__ sp_tab) {
  __shared__ __attribute__((aligned(16))) SoftplusNode s_lds[LDS ? TAB_NODES : 1];
  const SoftplusNode* s_tab = sp_tab;
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < TAB_NODES; i += 256) s_lds[i] = sp_tab[i];
    __syncthreads();
    s_tab = s_lds;
  }
  const long wave = (long)blockIdx.x * 4 + (long)(threadIdx.x >> 6);
  if (wave >= a.n_waves) return;  // whole waves only: the argument arrays are padded to a multiple of P
  const long base = wave * P + (long)(threadIdx.x & 63) * CPL;
  cell_op<OP>(a, base, wave, s_tab);
}

typedef void (*kernel_t)(const Args, const SoftplusNode*);
template <int OP>
kernel_t pick(bool lds) { return lds ? k_cell<OP, true> : k_cell<OP, false>; }

kernel_t kernel_of(int op, bool lds) {
  switch (op) {
    case OP_EXP_STRICT: return pick<OP_EXP_STRICT>(lds);
    case OP_LOG1P_STRICT: return pick<OP_LOG1P_STRICT>(lds);
    case OP_LOG_PLUS_STRICT: return pick<OP_LOG_PLUS_STRICT>(lds);
    case OP_PDF_STRICT: return pick<OP_PDF_STRICT>(lds);
    case OP_LOG_PLUS: return pick<OP_LOG_PLUS>(lds);
    case OP_SOFTPLUS: return pick<OP_SOFTPLUS>(lds);
    case OP_PDF: return pick<OP_PDF>(lds);
    case OP_EXP128: return pick<OP_EXP128>(lds);
    case OP_EMIS_FOLDED: return pick<OP_EMIS_FOLDED>(lds);
    case OP_LOG_PLUS_CERT: return pick<OP_LOG_PLUS_CERT>(lds);
  }
  return nullptr;
}

}  // namespace

// Runs operation `op` on n cells (a multiple of 448): allocates, uploads the tables and the n_in argument arrays, launches,
// downloads the n_out result arrays (and, where fb is given, the n / 448 per-wave fallback counts) and frees. Every HIP call's
// hipError_t goes into err[] in order (at most 64); returns how many were made, or -1 for a bad argument. The first failing
// step ends the run (what was allocated is still freed, those results are recorded too).
extern "C" int cm_run(int op, int lds, long n, int n_in, const double* const* in, int n_out, double* const* out, uint32_t* fb,
                      int* err) {
  if (op < 0 || op >= N_OPS || n <= 0 || n % P != 0 || n_in < 1 || n_in > MAX_IO || n_out < 1 || n_out > MAX_IO) return -1;
  int k = 0;
  bool ok = true;
  auto step = [&](hipError_t e) {
    err[k++] = (int)e;
    if (e != hipSuccess) ok = false;
    return e == hipSuccess;
  };
  std::vector<SoftplusNode> tab(TAB_NODES);  // dynamont_mi.cpp's upload, same functions, same order
  softplus_build_table(tab.data());
  exp128_build_table(reinterpret_cast<double*>(tab.data() + SP_NODES));
  std::memcpy(tab.data() + SP_NODES + EXP128_NODES, strict_exp_table(), STRICT_EXP_WORDS * 8);

  const size_t bytes = (size_t)n * sizeof(double), fb_bytes = (size_t)(n / P) * sizeof(uint32_t);
  void* d_tab = nullptr;
  void* d_in[MAX_IO] = {};
  void* d_out[MAX_IO] = {};
  void* d_fb = nullptr;
  Args a{};
  a.n_waves = n / P;
  if (ok) step(hipMalloc(&d_tab, sizeof(SoftplusNode) * tab.size()));
  for (int i = 0; ok && i < n_in; ++i) step(hipMalloc(&d_in[i], bytes));
  for (int i = 0; ok && i < n_out; ++i) step(hipMalloc(&d_out[i], bytes));
  if (ok && fb) step(hipMalloc(&d_fb, fb_bytes));
  if (ok) step(hipMemcpy(d_tab, tab.data(), sizeof(SoftplusNode) * tab.size(), hipMemcpyHostToDevice));
  for (int i = 0; ok && i < n_in; ++i) step(hipMemcpy(d_in[i], in[i], bytes, hipMemcpyHostToDevice));
  for (int i = 0; ok && i < n_out; ++i) step(hipMemset(d_out[i], 0xff, bytes));  // a cell nobody wrote reads as NaN
  if (ok && fb) step(hipMemset(d_fb, 0xff, fb_bytes));
  if (ok) {
    for (int i = 0; i < n_in; ++i) a.in[i] = static_cast<const double*>(d_in[i]);
    for (int i = 0; i < n_out; ++i) a.out[i] = static_cast<double*>(d_out[i]);
    a.fb = static_cast<uint32_t*>(d_fb);
    const unsigned groups = (unsigned)((a.n_waves + 3) / 4);
    hipLaunchKernelGGL(kernel_of(op, lds != 0), dim3(groups), dim3(256), 0, 0, a, static_cast<const SoftplusNode*>(d_tab));
    step(hipGetLastError());
  }
  if (ok) step(hipDeviceSynchronize());
  for (int i = 0; ok && i < n_out; ++i) step(hipMemcpy(out[i], d_out[i], bytes, hipMemcpyDeviceToHost));
  if (ok && fb) step(hipMemcpy(fb, d_fb, fb_bytes, hipMemcpyDeviceToHost));
  // frees are recorded whatever happened before
  if (d_fb) step(hipFree(d_fb));
  for (int i = 0; i < MAX_IO; ++i)
    if (d_out[i]) step(hipFree(d_out[i]));
  for (int i = 0; i < MAX_IO; ++i)
    if (d_in[i]) step(hipFree(d_in[i]));
  if (d_tab) step(hipFree(d_tab));
  return k;
}
