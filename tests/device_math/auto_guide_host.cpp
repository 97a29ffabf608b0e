// auto_guide_host.cpp -- test-only host driver (tests/test_auto_guide_host.py, tests/test_gpu_auto_guide.py): the pre-pass of
// dyn_batch_auto_guide walked by one thread, auto_guide_sequential of dynamont_amd/csrc/auto_guide_kernels.hpp -- the same
// per-cell arithmetic, argmax rule and centre update the kernel runs. Built with g++ -O2 -ffp-contract=off: the yardstick of the
// NumPy restatement (tests/auto_guide_cases.py) and, bit for bit, of k_auto_guide.
#define DYN_AUTO_GUIDE_MATH_ONLY
#include "auto_guide_kernels.hpp"

#include <vector>

// one read of T - 1 samples and N - 1 emission entries (entry n - 1 <-> lattice column n); guide: T - 1 entries. Returns 0, or
// -1 for an argument the sweep cannot take.
extern "C" int ag_host_guide(int T, int N, int hw, const double* sig, const double* mean, const double* stdev,
                             const double* neg_log_stdev, double m1, double e2, int32_t* guide) {
  if (T < 1 || N < 1 || hw < 1 || (T > 1 && (!sig || !guide)) || (N > 1 && (!mean || !stdev || !neg_log_stdev))) return -1;
  std::vector<dynmath::Emis> par((size_t)(N > 1 ? N - 1 : 0));
  for (int n = 0; n + 1 < N; ++n) par[(size_t)n] = dynmath::Emis{mean[n], 1.0 / stdev[n], neg_log_stdev[n], stdev[n]};
  std::vector<double> rows((size_t)4 * N);
  dynk::auto_guide_sequential(T, N, hw, sig, par.data(), m1, e2, guide, rows.data(), rows.data() + N, rows.data() + 2 * (size_t)N,
                              rows.data() + 3 * (size_t)N);
  return 0;
}
