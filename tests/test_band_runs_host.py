"""CPU: the run-length helpers of the sweeps (dynamont_amd/csrc/band_runs.hpp) compiled for the host with g++ must agree
with a row-by-row scan of the band centre int(float(t) * ratio), ratio = float(N) / float(T), for EVERY input: the sweeps
hand the band window over where the helpers say it moves, and a row off is a wrong lattice.

Each case is a read (T, N), a start row t and a limit; the scan walks from t until the centre changes. > 1e6 random
reads with T in 2 .. 200 000 and N / T drawn from the classes below, plus whole reads scanned at every row."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = r'''
#include "%s/dynamont_amd/csrc/band_runs.hpp"
// the scan: the expression of NT_aligner_api.cpp:100, one product, truncated
static inline int mid(int t, double ratio) { return (int)((double)t * ratio); }
static int scan_next_move(int t, double ratio, int limit) {
  for (int r = t; r < limit; ++r) if (mid(r + 1, ratio) != mid(r, ratio)) return r;
  return limit;
}
static int scan_run_first(int t, double ratio, int floor_row) {
  int q = t;
  while (q > floor_row && mid(q - 1, ratio) == mid(t, ratio)) --q;
  return q;
}
extern "C" {
int band_mid_of(int t, double ratio) { return dynband::band_mid(t, ratio); }
int next_move_row_of(int t, double ratio, double inv_ratio, int limit) { return dynband::next_move_row(t, ratio, inv_ratio, limit); }
int run_first_row_of(int t, double ratio, double inv_ratio, int floor_row) { return dynband::run_first_row(t, ratio, inv_ratio, floor_row); }
// cases whose helper result differs from the scan; the first offender's index -> *bad
long cmp_cases(const int* T, const int* N, const int* t, const int* span, long n, long* bad) {
  long c = 0;
  for (long i = 0; i < n; ++i) {
    const double ratio = (double)N[i] / (double)T[i], inv = 1.0 / ratio;
    const int up = t[i] + span[i] < T[i] ? t[i] + span[i] : T[i], down = t[i] - span[i] > 0 ? t[i] - span[i] : 0;
    const bool ok = dynband::next_move_row(t[i], ratio, inv, up) == scan_next_move(t[i], ratio, up) &&
                    dynband::run_first_row(t[i], ratio, inv, down) == scan_run_first(t[i], ratio, down);
    if (!ok) { if (!c) *bad = i; ++c; }
  }
  return c;
}
// one read, every row: the runs the forward sweep walks (blocks of 64 rows from row 1) and the backward sweep's
// (blocks of 64 rows down from row T - 2), each against the scan; a poor seed (inv scaled) must not matter
long cmp_read(int T, int N, double inv_scale) {
  const double ratio = (double)N / (double)T, inv = inv_scale / ratio;
  long c = 0;
  for (int tb = 1; tb < T; tb += 64) {
    const int tend = tb + (64 < T - tb ? 64 : T - tb);
    for (int t = tb; t < tend; ++t) c += dynband::next_move_row(t, ratio, inv, tend) != scan_next_move(t, ratio, tend);
  }
  for (int thi = T - 2; thi >= 0; thi -= 64) {
    const int tlo = thi - 63 > 0 ? thi - 63 : 0;
    for (int t = thi; t >= tlo; --t) c += dynband::run_first_row(t, ratio, inv, tlo) != scan_run_first(t, ratio, tlo);
  }
  return c;
}
}
''' % ROOT

ip = C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("bandruns")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    L.band_mid_of.argtypes = [C.c_int, C.c_double]
    L.next_move_row_of.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int]
    L.run_first_row_of.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int]
    L.cmp_cases.restype = C.c_long
    L.cmp_cases.argtypes = [ip, ip, ip, ip, C.c_long, C.POINTER(C.c_long)]
    L.cmp_read.restype = C.c_long
    L.cmp_read.argtypes = [C.c_int, C.c_int, C.c_double]
    return L


def _reads(rng, n):
    """(T, N) with T in 2 .. 200 000 and N / T of the classes: exactly 1, 1 - 1/T, 1/2, 2/3, 1/3, 0.1 +- 1e-12 (the nearest
    N / T on either side of 0.1, and T = 10 N itself), 1/64, 1/1000, T a multiple of N (every product t * ratio with t a
    multiple of T / N is an integer in exact arithmetic: within an ulp of one in fp64), and anything."""
    T = rng.integers(2, 200_001, n)
    cls = rng.integers(0, 12, n)
    N = np.empty(n, dtype=np.int64)
    for c in range(12):
        m = cls == c
        t = T[m]
        if c == 0:
            N[m] = t
        elif c == 1:
            N[m] = t - 1
        elif c == 2:
            t -= t % 2
            N[m] = t // 2
        elif c == 3:
            t -= t % 3
            t[t == 0] = 3
            N[m] = 2 * t // 3
        elif c == 4:
            t -= t % 3
            t[t == 0] = 3
            N[m] = t // 3
        elif c == 5:
            t -= t % 10
            t[t == 0] = 10
            N[m] = t // 10
        elif c == 6:
            N[m] = t // 10 + rng.integers(0, 2, len(t))   # the neighbours of 0.1 this T admits
        elif c == 7:
            t -= t % 64
            t[t == 0] = 64
            N[m] = t // 64
        elif c == 8:
            t -= t % 1000
            t[t == 0] = 1000
            N[m] = t // 1000
        elif c == 9:
            k = rng.integers(1, 200, len(t))
            nn = np.maximum(t // k, 1)
            T[m] = t = nn * k                             # T a multiple of N
            N[m] = nn
            continue
        else:
            N[m] = rng.integers(1, t + 1)
        T[m] = t
    N = np.clip(N, 1, T)
    return T.astype(np.int32), N.astype(np.int32)


def test_helpers_equal_the_row_by_row_scan(lib):
    rng = np.random.default_rng(20261017)
    n = 1_200_000
    T, N = _reads(rng, n)
    t = (rng.random(n) * T).astype(np.int32)                      # 0 .. T - 1
    # start rows on and next to the steps as well: t * ratio integral, one before, one after
    on = rng.random(n) < 0.4
    j = (rng.random(n) * N).astype(np.int64)
    step = np.minimum((j * T.astype(np.int64) + N - 1) // N, T - 1) + rng.integers(-1, 2, n)
    t = np.where(on, np.clip(step, 0, T - 1), t).astype(np.int32)
    span = rng.choice(np.array([1, 2, 63, 64, 65, 1000, 200_000], dtype=np.int32), n)
    arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (T, N, t, span)]
    bad = C.c_long(-1)
    c = lib.cmp_cases(*[a.ctypes.data_as(ip) for a in arrs], C.c_long(n), C.byref(bad))
    i = bad.value
    assert c == 0, (c, int(T[i]), int(N[i]), int(t[i]), int(span[i]))
    # the scan above is C++: its band centre is Python's int(float(t) * ratio) on a sample of the same cases
    for i in rng.integers(0, n, 20_000):
        ratio = float(N[i]) / float(T[i])
        assert lib.band_mid_of(int(t[i]), ratio) == int(float(t[i]) * ratio)


@pytest.mark.parametrize("T,N", [(2, 1), (2, 2), (3, 2), (5, 3), (65, 33), (129, 65), (1001, 501), (1000, 500), (999, 666), (999, 333),
                                 (20001, 2001), (20000, 2000), (19999, 2000), (6400, 100), (6401, 100), (200000, 200),
                                 (200000, 3), (131072, 1), (4097, 4096), (4096, 4096), (199999, 100000)])
def test_whole_reads_every_row_and_a_poor_seed(lib, T, N):
    """Every row of a read as a run start, in the sweeps' own 64-row blocks; the prediction only seeds the search, so a
    seed off by a factor (or useless: 0, inf, nan) costs steps, never the result. Python's own scan beside it for the
    forward runs of the small reads."""
    for scale in (1.0, 1.0 + 1e-9, 0.97, 1.5, 0.0, float("inf"), float("nan")):
        if T > 25_000 and scale not in (1.0, 1.0 + 1e-9):
            continue   # (a useless seed walks row by row: quadratic in the run length)
        assert lib.cmp_read(T, N, scale) == 0, scale
    if T <= 1001:
        ratio = float(N) / float(T)
        for t in range(1, T):
            limit = min(T, t + 64)
            want = next((r for r in range(t, limit) if int(float(r + 1) * ratio) != int(float(r) * ratio)), limit)
            assert lib.next_move_row_of(t, ratio, 1.0 / ratio, limit) == want, t
