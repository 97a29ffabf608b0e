// preprocess_kernels.hpp -- P1/P2 on the device: k_normalise, window_median, k_hampel, the sliced launches (preprocess_t)
// and the dispatch over the eight (REAL, RAW, calibration) instantiations (launch_preprocess), text as it stood in
// nt_kernels.hip. Included by nt_kernels.hip and by tests/device_math/preprocess.hip, which hands launch_preprocess host
// arrays and compares every output sample with the NumPy restatement (tests/test_gpu_preprocess_kernels.py).
// The kernels are ordinary (non-inline) definitions: one translation unit per binary includes this file.
#pragma once

#include <algorithm>

#include "nt_kernels.hpp"
#include "segment_kernels.hpp"  // MAX_GRID_Y

namespace dynk {

// ---------------------------------------------------------------------------------------------
// P1/P2 on the device: the per-read preprocessing of segment.py:146-153 / train.py:163-170.
//   x = REAL(raw[i]); x -= shift; x /= scale            (REAL = double for dynamont-resquiggle,
//   hampel(x, W, n_sigmas)   (utils.py:16-43)             float for dynamont-train, whose signal
// Windows are taken from the UNFILTERED normalised signal; centres W/2 .. W/2 + nwin - 1 with        stays float32)
// nwin = S - W - (W even); a centre is replaced by the window median when
// |x - med| > n_sigmas * (1.4826 * MAD). Every operation is a single IEEE op in the reference's
// order, so the result is bit-identical to the NumPy code (tests/test_gpu_preprocess.py).
// ---------------------------------------------------------------------------------------------
// CAL: the samples are int16 ADC counts with the read's pod5 calibration (pod5_io.py:6-16, `signal_pa`): picoampere
// = (float(adc) + offset) * scale in float32, one IEEE operation each -- the value the reference's reader hands over.
template <class REAL, class RAW, bool CAL>
__global__ void k_normalise(const RAW* __restrict__ raw, const uint64_t* __restrict__ offs,
                            const double* __restrict__ shift, const double* __restrict__ scale,
                            const float* __restrict__ cal_offset, const float* __restrict__ cal_scale,
                            REAL* __restrict__ norm, int n_reads) {
  const int r = blockIdx.y;
  if (r >= n_reads) return;
  const uint64_t a = offs[r], b = offs[r + 1];
  const REAL sh = (REAL)shift[r], sc = (REAL)scale[r];
  const float co = CAL ? cal_offset[r] : 0.0f, cs = CAL ? cal_scale[r] : 1.0f;
  for (uint64_t i = a + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < b; i += (uint64_t)gridDim.x * blockDim.x) {
    REAL x;
    if (CAL) {
      float pa = (float)raw[i] + co;
      pa = pa * cs;
      x = (REAL)pa;
    } else {
      x = (REAL)raw[i];
    }
    x = x - sh;
    norm[i] = x / sc;
  }
}

template <class REAL, int MAXW>
__device__ __forceinline__ REAL window_median(REAL (&w)[MAXW], int W) {
  for (int i = 1; i < W; ++i) {  // insertion sort of <= MAXW values
    const REAL v = w[i];
    int j = i - 1;
    while (j >= 0 && w[j] > v) {
      w[j + 1] = w[j];
      --j;
    }
    w[j + 1] = v;
  }
  return (W & 1) ? w[W / 2] : (w[W / 2 - 1] + w[W / 2]) / (REAL)2;
}

template <class REAL>
__global__ void k_hampel(const REAL* __restrict__ norm, const uint64_t* __restrict__ offs,
                         double* __restrict__ out, int n_reads, int W, double n_sigmas) {
  constexpr int MAXW = 16;
  const int r = blockIdx.y;
  if (r >= n_reads) return;
  const uint64_t a = offs[r], S = offs[r + 1] - offs[r];
  const long nwin = (S <= (uint64_t)W) ? 0 : (long)S - W - ((W & 1) ? 0 : 1);
  const int half = W / 2;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < S; i += (uint64_t)gridDim.x * blockDim.x) {
    REAL x = norm[a + i];
    const long wi = (long)i - half;  // window index of this centre
    if (wi >= 0 && wi < nwin) {
      REAL w[MAXW], d[MAXW];
      for (int q = 0; q < W; ++q) w[q] = norm[a + wi + q];
      for (int q = 0; q < W; ++q) d[q] = w[q];
      const REAL med = window_median<REAL, MAXW>(d, W);
      for (int q = 0; q < W; ++q) d[q] = fabs(w[q] - med);
      const REAL mad = window_median<REAL, MAXW>(d, W);
      const REAL sigma = (REAL)1.4826 * mad;
      if (fabs(x - med) > (REAL)n_sigmas * sigma) x = med;
    }
    out[a + i] = (double)x;
  }
}


template <class REAL, class RAW, bool CAL>
static void preprocess_t(const RAW* raw, const uint64_t* offs, const double* shift, const double* scale,
                         const float* cal_offset, const float* cal_scale, void* norm_tmp, double* out, int n_reads,
                         uint64_t max_len, int W, double ns, hipStream_t s) {
  const int bx = (int)std::min<uint64_t>(1024, (max_len + 255) / 256);
  for (int r0 = 0; r0 < n_reads; r0 += MAX_GRID_Y) {  // offs hold absolute sample positions: slices just shift the read index
    const int nr = std::min(MAX_GRID_Y, n_reads - r0);
    hipLaunchKernelGGL((k_normalise<REAL, RAW, CAL>), dim3(bx ? bx : 1, nr), dim3(256), 0, s, raw, offs + r0, shift + r0,
                       scale + r0, CAL ? cal_offset + r0 : nullptr, CAL ? cal_scale + r0 : nullptr, (REAL*)norm_tmp, nr);
    hipLaunchKernelGGL((k_hampel<REAL>), dim3(bx ? bx : 1, nr), dim3(256), 0, s, (const REAL*)norm_tmp, offs + r0, out,
                       nr, W, ns);
  }
}

void launch_preprocess(const void* raw, int raw_dtype, int compute_f32, const uint64_t* offs,
                       const double* shift, const double* scale, const float* cal_offset, const float* cal_scale,
                       void* norm_tmp, double* out, int n_reads, uint64_t max_len, int W, double n_sigmas, hipStream_t s) {
  if (n_reads <= 0) return;
#define DYN_PRE(REAL, RAW, CAL) \
  preprocess_t<REAL, RAW, CAL>((const RAW*)raw, offs, shift, scale, cal_offset, cal_scale, norm_tmp, out, n_reads, max_len, W, n_sigmas, s)
  if (compute_f32) {
    if (raw_dtype == 0) DYN_PRE(float, float, false);
    else if (raw_dtype == 1) DYN_PRE(float, int16_t, false);
    else if (raw_dtype == 3) DYN_PRE(float, int16_t, true);
    else DYN_PRE(float, double, false);
  } else {
    if (raw_dtype == 0) DYN_PRE(double, float, false);
    else if (raw_dtype == 1) DYN_PRE(double, int16_t, false);
    else if (raw_dtype == 3) DYN_PRE(double, int16_t, true);
    else DYN_PRE(double, double, false);
  }
#undef DYN_PRE
}

}  // namespace dynk
