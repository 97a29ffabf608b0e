// site_mixture_host.cpp -- test-only (tests/site_mixture_cases.py): the strict exp of dp_math_strict.hpp built for the HOST with
// g++ -O2 -ffp-contract=off and loaded with ctypes, so that the Python restatement of the per-site mixture fit uses the exp the
// kernel uses (exp_strict_vec over the library's own table) and does not depend on the host's libm.
#include "dp_math_strict.hpp"

extern "C" double exp_strict(double x) {
  const double a[1] = {x};
  double o[1];
  dynmath::exp_strict_vec<1>(a, o, dynmath::strict_exp_table());
  return o[0];
}

extern "C" void exp_strict_n(const double* x, double* out, long n) {
  for (long i = 0; i < n; ++i) out[i] = exp_strict(x[i]);
}
