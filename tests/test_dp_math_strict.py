"""CPU: the strict-mode arithmetic (dynamont_amd/csrc/dp_math_strict.hpp) compiled for the host with g++ must give
the SAME BITS as the libm the compiled reference links (glibc: table-driven exp, fdlibm log1p) and as the
reference's log_normal_pdf / logPlus expressions (src/cpp/aligner.cpp:276-292), on > 1e7 arguments.

The comparison partner is the libm of the machine the test runs on. The restatement follows glibc 2.35's x86-64
FMA variant of exp (what oracle/_ref uses on any host with FMA); on a host whose libm is something else the test
skips instead of failing."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = r'''
#include "%s/dynamont_amd/csrc/dp_math_strict.hpp"
#include <cmath>
#include <cstring>
using namespace dynmath;
static inline bool same(double a, double b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }
static double ref_log_plus(double x, double y) {   // aligner.cpp:276-285
  if (std::isinf(x)) return y;
  if (std::isinf(y)) return x;
  if (x < y) { const double t = x; x = y; y = t; }
  return x + std::log1p(std::exp(y - x));
}
static double ref_pdf(double x, double mean, double sd) {   // aligner.cpp:287-292
  const double diff = x - mean; const double z = diff / sd;
  return -0.5 * z * z - std::log(sd) - 0.5 * std::log(2.0 * M_PI);
}
extern "C" {
// number of arguments whose result differs from libm's in any bit; first offender -> *bad
long cmp_exp(const double* x, long n, double* bad) {
  long c = 0; const uint64_t* T = strict_exp_table();
  for (long i = 0; i + 7 <= n; i += 7) {
    double a[7], o[7];
    for (int j = 0; j < 7; ++j) a[j] = x[i + j];
    exp_strict_vec<7>(a, o, T);
    for (int j = 0; j < 7; ++j) if (!same(o[j], std::exp(a[j]))) { if (!c) *bad = a[j]; ++c; }
  }
  return c;
}
long cmp_log1p(const double* x, long n, double* bad) {
  long c = 0;
  for (long i = 0; i + 7 <= n; i += 7) {
    double a[7], o[7];
    for (int j = 0; j < 7; ++j) a[j] = x[i + j];
    log1p_strict_vec<7>(a, o);
    for (int j = 0; j < 7; ++j) if (!same(o[j], std::log1p(a[j]))) { if (!c) *bad = a[j]; ++c; }
  }
  return c;
}
long cmp_log_plus(const double* x, const double* y, long n, double* bad) {
  long c = 0; const uint64_t* T = strict_exp_table();
  for (long i = 0; i + 7 <= n; i += 7) {
    double a[7], b[7], o[7];
    for (int j = 0; j < 7; ++j) { a[j] = x[i + j]; b[j] = y[i + j]; }
    log_plus_strict_vec<7>(a, b, o, T);
    for (int j = 0; j < 7; ++j) if (!same(o[j], ref_log_plus(a[j], b[j]))) { if (!c) { bad[0] = a[j]; bad[1] = b[j]; } ++c; }
  }
  return c;
}
long cmp_pdf(const double* x, const double* mean, const double* sd, long n, double* bad) {
  long c = 0;
  for (long i = 0; i + 7 <= n; i += 7) {
    EmisV<7> p; double o[7];
    for (int j = 0; j < 7; ++j) { Emis e = make_emis(mean[i + j], sd[i + j], std::log(sd[i + j])); p.set(j, e); p.inv_stdev[j] = e.stdev; }
    for (int j = 0; j < 7; ++j) {
      log_normal_pdf_strict_vec<7>(x[i + j], p, o);
      const double want = ref_pdf(x[i + j], mean[i + j], sd[i + j]);
      if (!same(o[j], want) || !same(log_normal_pdf_strict(x[i + j], make_emis(mean[i + j], sd[i + j], std::log(sd[i + j]))), want)) { if (!c) *bad = x[i + j]; ++c; }
    }
  }
  return c;
}
}
''' % ROOT

dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("dpstrict")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    for f in (L.cmp_exp, L.cmp_log1p, L.cmp_log_plus, L.cmp_pdf):
        f.restype = C.c_long
    # is this host's libm the one the restatement follows? 16 probes in the range where the FMA and non-FMA
    # variants of glibc's exp differ most often would not tell; compare a dense sample instead
    x = -np.random.default_rng(99).uniform(0, 40, 7 * 3000)
    bad = C.c_double()
    if L.cmp_exp(x.ctypes.data_as(dp), C.c_long(len(x)), C.byref(bad)) > 20:
        pytest.skip("this host's libm exp is not glibc's table-driven FMA variant")
    return L


def _seven(a):
    return np.ascontiguousarray(a[: len(a) // 7 * 7], dtype=np.float64)


def test_exp_bits_equal_libm(lib):
    rng = np.random.default_rng(1)
    x = _seven(np.concatenate([
        -rng.uniform(0, 50, 6_000_000), -rng.uniform(0, 50, 2_000_000) * rng.uniform(0, 1, 2_000_000) ** 3,
        -rng.uniform(0, 800, 1_500_000), -10.0 ** rng.uniform(-300, 3.2, 500_000),
        [0.0, -0.0, -1e-320, -2.0 ** -54, -2.0 ** -55, -511.99999, -512.0, -512.0000001, -708.3, -708.5, -744.9, -745.2, -1023.9,
         -1024.0, -1e300, -np.inf, -0.6931471805599453, -1.0]]))
    bad = C.c_double()
    n = lib.cmp_exp(x.ctypes.data_as(dp), C.c_long(len(x)), C.byref(bad))
    assert n == 0, (n, bad.value)


def test_log1p_bits_equal_libm(lib):
    rng = np.random.default_rng(2)
    x = _seven(np.concatenate([
        rng.uniform(0, 1, 4_000_000), np.exp(-rng.uniform(0, 50, 4_000_000)), np.exp(-rng.uniform(0, 2, 2_000_000)),
        np.exp(-rng.uniform(0, 800, 500_000)), 1.0 - 10.0 ** rng.uniform(-16, -3, 500_000),
        [0.0, 1.0, 2.0 ** -54, 2.0 ** -29, np.nextafter(2.0 ** -29, 0), np.nextafter(2.0 ** -54, 0), 5e-324,
         0.41421353816986084, np.nextafter(0.41421353816986084, 0), 0.41421356237309503, 0.4142135623730951, 0.5,
         np.nextafter(1.0, 0), 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -19, 1.0 - 2.0 ** -21]]))
    bad = C.c_double()
    n = lib.cmp_log1p(x.ctypes.data_as(dp), C.c_long(len(x)), C.byref(bad))
    assert n == 0, (n, bad.value)


def test_log_plus_bits_equal_reference_expression(lib):
    rng = np.random.default_rng(3)
    n = 7 * 600_000
    x = rng.uniform(-60000, 50, n)
    y = x + np.where(rng.random(n) < 0.5, rng.uniform(-45, 45, n), rng.standard_normal(n) * 10.0 ** rng.uniform(-9, 3, n))
    # special operands: -inf on either or both sides, equal operands, a zero maximum with a far smaller minimum
    x[:7] = [-np.inf, -np.inf, 3.0, -5.0, 0.0, 0.0, -7.25]
    y[:7] = [-np.inf, -2.5, -np.inf, -5.0, -600.0, -720.0, -7.25]
    bad = (C.c_double * 2)()
    c = lib.cmp_log_plus(x.ctypes.data_as(dp), y.ctypes.data_as(dp), C.c_long(n), bad)
    assert c == 0, (c, bad[0], bad[1])


def test_log_normal_pdf_bits_equal_reference_expression(lib):
    rng = np.random.default_rng(4)
    n = 7 * 300_000
    mean = rng.standard_normal(n) * 2
    sd = rng.uniform(0.05, 3.0, n)
    x = mean + sd * rng.standard_normal(n) * rng.choice([0.1, 1.0, 6.0, 40.0], n)
    bad = C.c_double()
    c = lib.cmp_pdf(x.ctypes.data_as(dp), mean.ctypes.data_as(dp), sd.ctypes.data_as(dp), C.c_long(n), C.byref(bad))
    assert c == 0, (c, bad.value)


# ---- certified arithmetic (round 4) -----------------------------------------------------------------------------------
CERT_SRC = r'''
#include "%s/dynamont_amd/csrc/dp_math_strict.hpp"
#include <cmath>
#include <cstring>
#include <vector>
using namespace dynmath;
static inline bool same(double a, double b) { return bits_of(a) == bits_of(b) || (a != a && b != b); }
static double ref_log_plus(double x, double y) {   // aligner.cpp:276-285
  if (std::isinf(x)) return y;
  if (std::isinf(y)) return x;
  if (x < y) { const double t = x; x = y; y = t; }
  return x + std::log1p(std::exp(y - x));
}
static double ref_pdf(double x, double mean, double sd) {   // aligner.cpp:287-292
  const double diff = x - mean; const double z = diff / sd;
  return -0.5 * z * z - std::log(sd) - 0.5 * std::log(2.0 * M_PI);
}
struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  double uni() { return (double)(next() >> 11) * 0x1p-53; }
};
static std::vector<SoftplusNode> TAB;
static const SoftplusNode* tab() { if (TAB.empty()) { TAB.resize(SP_NODES); softplus_build_table(TAB.data()); } return TAB.data(); }
extern "C" {
// quotients by the divisors sd[0..nsd): `per` dividends each (random significands and exponents around the divisor's
// scale, plus dividends built to land next to rounding boundaries of the quotient). Returns the number of wrong bits.
long cmp_div(const double* sd, long nsd, long per, uint64_t seed, double* bad) {
  Rng g{seed}; long c = 0;
  for (long i = 0; i < nsd; ++i) {
    const double b = sd[i], y = 1.0 / b;
    for (long k = 0; k < per; ++k) {
      double a;
      const uint64_t r = g.next();
      if (k & 1) {  // a = b x (a quotient with a random significand) +- a few ulps: near-exact quotients are the hard cases
        const double q = std::ldexp(1.0 + g.uni(), (int)(r %% 40) - 20);
        a = q * b;
        a = std::nextafter(a, (r & 64) ? 1e308 : -1e308);
      } else {
        a = std::ldexp(1.0 + g.uni(), (int)(r %% 90) - 60) * ((r & 128) ? -1.0 : 1.0);
      }
      if (!same(div_by_const(a, b, y), a / b)) { if (!c) { bad[0] = a; bad[1] = b; } ++c; }
      if (!same(div_by_const4(a, b, y, recip_lo(b, y)), a / b)) { if (!c) { bad[0] = a; bad[1] = b; } ++c; }   // round 6: four operations
    }
  }
  return c;
}
long cmp_pdf_cert(const double* x, const double* mean, const double* sd, long n, double* bad) {
  long c = 0;
  for (long i = 0; i + 7 <= n; i += 7) {
    EmisV<7> p; double st[7], o[7];
    for (int j = 0; j < 7; ++j) { Emis e = make_emis(mean[i + j], sd[i + j], std::log(sd[i + j])); p.set(j, e); st[j] = e.stdev; }
    for (int j = 0; j < 7; ++j) {
      double yl[7], o4[7];
      for (int k = 0; k < 7; ++k) yl[k] = recip_lo(st[k], p.inv_stdev[k]);
      log_normal_pdf_cert4_vec<7>(x[i + j], p, st, yl, o4);
      log_normal_pdf_cert_vec<7>(x[i + j], p, st, o);
      if (!same(o4[j], o[j])) { if (!c) *bad = x[i + j]; ++c; }
      const double want = ref_pdf(x[i + j], mean[i + j], sd[i + j]);
      if (!same(o[j], want) || !same(log_normal_pdf_cert(x[i + j], make_emis(mean[i + j], sd[i + j], std::log(sd[i + j]))), want)) { if (!c) *bad = x[i + j]; ++c; }
    }
  }
  return c;
}
// n random (hi, d) pairs: |hi| log-uniform in [1e-3, 1e6] (or exactly 0 / tiny now and then), d by `kind`:
//   0: -uniform(0, 45); 1: -uniform(0,1)^4 x 3 (the softplus near ln 2: the widest intervals); 2: -10^uniform(-12, 2)
// out[0] = sums whose certificate held but differ from the reference expression (must be 0), out[1] = ambiguous sums,
// out[2] = certified results of the full function (fallback included) that differ (must be 0)
void cert_log_plus(long n, int kind, uint64_t seed, long* out, double* bad) {
  Rng g{seed}; const SoftplusNode* T = tab(); const uint64_t* E = strict_exp_table();
  long wrong = 0, amb = 0, wrong_full = 0;
  for (long i = 0; i < n; ++i) {
    const double mag = std::pow(10.0, -3.0 + 9.0 * g.uni());
    double hi = -mag;
    const uint64_t r = g.next();
    if ((r & 1023) == 0) hi = 0.0;
    if ((r & 1023) == 1) hi = mag * 1e-12;
    double d;
    if (kind == 0) d = -45.0 * g.uni();
    else if (kind == 1) { const double u = g.uni(); d = -3.0 * u * u * u * u; }
    else d = -std::pow(10.0, -12.0 + 14.0 * g.uni());
    double lo = hi + d;
    double x = (r & 2048) ? hi : lo, y = (r & 2048) ? lo : hi;
    const double want = ref_log_plus(x, y);
    double a[1] = {x}, b[1] = {y}, l[1], h[1];
    SoftplusLookup<1> L;
    log_plus_issue<1>(a, b, L, T);
    log_plus_finish_cert<1>(L, l, h);
    if (l[0] == h[0]) { if (!same(l[0], want)) { if (!wrong) { bad[0] = x; bad[1] = y; } ++wrong; } }
    else ++amb;
    long dummy = 0;
    if (!same(log_plus_cert(x, y, T, E, &dummy), want)) ++wrong_full;
  }
  out[0] = wrong; out[1] = amb; out[2] = wrong_full;
}
// max over n arguments d of |table softplus - log1p(exp(d))| / log1p(exp(d)), in units of 2^-52; *absmax_below: the
// largest glibc value for d < -39.99 (where the table returns 0: the last node and everything below it)
double softplus_gap(long n, uint64_t seed, double* absmax_below) {
  Rng g{seed}; const SoftplusNode* T = tab(); double worst = 0.0, below = 0.0;
  for (long i = 0; i < n; i += 7) {
    double d[7], o[7];
    for (int j = 0; j < 7; ++j) { const double u = g.uni(); d[j] = (g.next() & 1) ? -41.0 * u : -41.0 * u * u * u; }
    double dd[7]; std::memcpy(dd, d, sizeof d);
    softplus_table_vec<7>(dd, o, T);
    for (int j = 0; j < 7; ++j) {
      const double want = std::log1p(std::exp(d[j]));
      if (d[j] < -39.99) { if (want > below) below = want; continue; }  // the last node holds (0, 0): the absolute term's region
      const double rel = std::fabs(o[j] - want) / want * 0x1p52;
      if (rel > worst) worst = rel;
    }
  }
  *absmax_below = below;
  return worst;
}

// ---- plain evaluations, 7 cells at a time: the host side of tests/test_gpu_cell_math.py, which runs the same headers on the
// device (tests/device_math/cell_math.hip, same operations in the same order) and compares bit patterns ----
#define SEVENS(i) for (long i = 0; i + 7 <= n; i += 7)
#define LOAD7(v, src) for (int j = 0; j < 7; ++j) v[j] = src[i + j]
#define STORE7(dst, v) for (int j = 0; j < 7; ++j) dst[i + j] = v[j]
static const double* exp128() { static double T[EXP128_SIZE]; static bool init = false; if (!init) { exp128_build_table(T); init = true; } return T; }
void ev_libm_exp(const double* x, double* o, long n) { for (long i = 0; i < n; ++i) o[i] = std::exp(x[i]); }
void ev_ref_log_plus(const double* x, const double* y, double* o, long n) { for (long i = 0; i < n; ++i) o[i] = ref_log_plus(x[i], y[i]); }
void ev_exp_strict(const double* x, double* o, long n) {
  SEVENS(i) { double a[7], r[7]; LOAD7(a, x); exp_strict_vec<7>(a, r, strict_exp_table()); STORE7(o, r); } }
void ev_log1p_strict(const double* x, double* o, long n) {
  SEVENS(i) { double a[7], r[7]; LOAD7(a, x); log1p_strict_vec<7>(a, r); STORE7(o, r); } }
void ev_log_plus_strict(const double* x, const double* y, double* o, double* o_from, long n) {
  SEVENS(i) {
    double a[7], b[7], r[7]; LOAD7(a, x); LOAD7(b, y);
    log_plus_strict_vec<7>(a, b, r, strict_exp_table()); STORE7(o, r);
    SoftplusLookup<7> L; log_plus_issue<7>(a, b, L, tab());
    for (int j = 0; j < 7; ++j) o_from[i + j] = log_plus_strict_from(L.hi[j], L.diff[j], strict_exp_table());
  } }
// inv = RN(1 / sd) and nls = -log(sd) come from the caller, as the kernels get them from the model load
void ev_pdf_strict(const double* x, const double* mean, const double* sd, const double* inv, const double* nls, double* o_strict,
                   double* o_cert, double* o_cert4, double* o_q5, double* o_q4, double* o_q, long n) {
  SEVENS(i) {
    EmisV<7> p; double st[7], yl[7], o[7];
    for (int j = 0; j < 7; ++j) {
      const Emis e{mean[i + j], inv[i + j], nls[i + j], sd[i + j]};
      p.set(j, e); st[j] = e.stdev; yl[j] = recip_lo(e.stdev, e.inv_stdev);
      o_strict[i + j] = log_normal_pdf_strict(x[i + j], e);
      const double d = x[i + j] - e.mean;
      o_q5[i + j] = div_by_const(d, e.stdev, e.inv_stdev);
      o_q4[i + j] = div_by_const4(d, e.stdev, e.inv_stdev, yl[j]);
      o_q[i + j] = d / e.stdev;
    }
    for (int j = 0; j < 7; ++j) {
      log_normal_pdf_cert_vec<7>(x[i + j], p, st, o); o_cert[i + j] = o[j];
      log_normal_pdf_cert4_vec<7>(x[i + j], p, st, yl, o); o_cert4[i + j] = o[j];
    }
  } }
void ev_log_plus_table(const double* x, const double* y, double* o5, double* o3, long n) {
  SEVENS(i) {
    double a[7], b[7], r[7]; LOAD7(a, x); LOAD7(b, y);
    SoftplusLookup<7> L; log_plus_issue<7>(a, b, L, tab());
    log_plus_finish<7>(L, r); STORE7(o5, r);
    log_plus_finish3<7>(L, r); STORE7(o3, r);
  } }
void ev_softplus_table(const double* d, double* o5, double* o3, long n) {
  SEVENS(i) {
    double a[7], r[7]; LOAD7(a, d);
    softplus_table_vec<7>(a, r, tab()); STORE7(o5, r);
    softplus_table3_vec<7>(a, r, tab()); STORE7(o3, r);
  } }
void ev_pdf_vec(const double* x, const double* mean, const double* inv, const double* nls, double* o, long n) {
  SEVENS(i) {
    EmisV<7> p; double r[7];
    for (int j = 0; j < 7; ++j) p.set(j, Emis{mean[i + j], inv[i + j], nls[i + j], 0.0});
    for (int j = 0; j < 7; ++j) { log_normal_pdf_vec<7>(x[i + j], p, r); o[i + j] = r[j]; }
  } }
// the training sweep's exponential, and its value clipped to 1 as forward_train_chain clips it
void ev_exp128(const double* x, double* o, double* o_min, long n) {
  SEVENS(i) {
    double a[7], r[7]; LOAD7(a, x);
    exp_table128_vec<7>(a, r, exp128()); STORE7(o, r);
    for (int j = 0; j < 7; ++j) o_min[i + j] = min_hw(r[j], 1.0);
  } }
// the training sweep's folded emission (dp_cell.hpp, set_emis<ARITH_FOLDED> + emission_vec<ARITH_FOLDED>: device code, so its
// preparatory product and difference and its three operations are repeated here): ln P = ln K - u^2, u = (x - mean) c,
// c = 1 / (stdev sqrt 2)
void ev_emis_folded(const double* x, const double* mean, const double* inv, const double* nls, double* o, long n) {
  for (long i = 0; i < n; ++i) {
    const double c = inv[i] * 0x1.6a09e667f3bcdp-1, k = nls[i] - HALF_LOG_2PI;
    double u = x[i] - mean[i];
    u = u * c;
    o[i] = fma_(-u, u, k);
  } }
// the certified logPlus cell by cell: o = its result (fallback included), o_lo = the lower end of the certificate (what a
// kernel without the fallback would keep), amb = 1 where the certificate failed
void ev_log_plus_cert(const double* x, const double* y, double* o, double* o_lo, unsigned char* amb, long n) {
  for (long i = 0; i < n; ++i) {
    double a[1] = {x[i]}, b[1] = {y[i]}, l[1], h[1];
    SoftplusLookup<1> L;
    log_plus_issue<1>(a, b, L, tab());
    log_plus_finish_cert<1>(L, l, h);
    o_lo[i] = l[0];
    amb[i] = !(l[0] == h[0]);
    o[i] = log_plus_cert(x[i], y[i], tab(), strict_exp_table(), nullptr);
  } }
}
''' % ROOT


@pytest.fixture(scope="module")
def cert(tmp_path_factory, lib):  # `lib` first: skips on a host whose libm is not the one restated
    d = tmp_path_factory.mktemp("dpcert")
    src = d / "c.cpp"
    src.write_text(CERT_SRC)
    so = d / "libc.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    L.cmp_div.restype = C.c_long
    L.cmp_pdf_cert.restype = C.c_long
    L.softplus_gap.restype = C.c_double
    return L


def _model_stdevs():
    """Every distinct stdev of the model files this build is tested with: the synthetic tables (constant stdev by
    construction) and the value ranges real ONT tables use (three decimals, 0.5 .. 30 pA / 0.05 .. 0.5 normalised)."""
    rng = np.random.default_rng(11)
    return np.unique(np.concatenate([[0.15, 0.25, 1.0], np.round(rng.uniform(0.05, 0.6, 2000), 6),
                                     np.round(rng.uniform(0.5, 30.0, 2000), 3), rng.uniform(0.01, 50.0, 1000)]))


def test_division_by_constant_equals_ieee_division(cert):
    sd = np.ascontiguousarray(_model_stdevs())
    per = 100_000_000 // len(sd) + 1
    bad = (C.c_double * 2)()
    c = cert.cmp_div(sd.ctypes.data_as(dp), C.c_long(len(sd)), C.c_long(per), C.c_uint64(5), bad)
    assert c == 0, (c, bad[0], bad[1])  # >= 1e8 (dividend, stdev) pairs, 0 differing bits


def test_certified_emission_bits_equal_reference_expression(cert):
    rng = np.random.default_rng(4)
    n = 7 * 300_000
    mean = rng.standard_normal(n) * 2
    sd = rng.choice(_model_stdevs(), n)
    x = mean + sd * rng.standard_normal(n) * rng.choice([0.1, 1.0, 6.0, 40.0], n)
    bad = C.c_double()
    c = cert.cmp_pdf_cert(x.ctypes.data_as(dp), mean.ctypes.data_as(dp), sd.ctypes.data_as(dp), C.c_long(n), C.byref(bad))
    assert c == 0, (c, bad.value)


def test_table_softplus_within_the_certificates_interval(cert):
    below = C.c_double()
    worst = cert.softplus_gap(C.c_long(7 * 14_300_000), C.c_uint64(6), C.byref(below))
    # the certificate allows 4 x 2^-52 relative (minus 0.5 for its own rounding) and 2^-57 absolute below d = -40
    assert worst <= 2.0, worst   # observed 1.0: the two never differ by more than one unit in the last place
    assert below.value < 2.0 ** -57, below.value


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_certified_log_plus_never_differs_from_reference(cert, kind):
    out = (C.c_long * 3)()
    bad = (C.c_double * 2)()
    n = 34_000_000
    cert.cert_log_plus(C.c_long(n), C.c_int(kind), C.c_uint64(100 + kind), out, bad)
    assert out[0] == 0, ("a certified sum differs from the reference", out[0], bad[0], bad[1])
    assert out[2] == 0, ("certified logPlus with fallback differs", out[2])
    # |hi| is log-uniform over 1e-3 .. 1e6 here and every sum with |hi| < ~1 is ambiguous by the absolute term; what the
    # DP's own operands give is measured by tests/tie_parity.py mode 7 (profiles/r04/cert_ambiguity.json)
    assert out[1] < 0.5 * n
