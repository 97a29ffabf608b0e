"""CPU: the address runs of the sweeps (dynamont_amd/csrc/band_runs.hpp: fwd_run_end, fwd_address_run_end,
fwd_fetch_advances, bwd_run_first) compiled for the host with g++.

Inside a run the sweeps do not look a row's address up: they add a constant to the previous row's. The forward sweep has two
cursors, the row t it writes and the row min(t + 1 + RING_D, T) it fetches; the backward sweep has one. A run that spans a
page crossing of a cursor, or the row at which the fetch starts to repeat row T, writes or reads another read's lattice.

The walk below is the kernels' own (64-row blocks, runs inside them, running values recomputed where a run starts) over a
page table of random page numbers; every row's running addresses must equal the looked-up ones, the runs must tile the rows,
and each run must end exactly where the row-by-row scan ends it."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT

RING_D = 4
AHEAD = 1 + RING_D

SRC = r'''
#include <cstdint>
#include "%s/dynamont_amd/csrc/band_runs.hpp"
static inline int mid(int t, double ratio) { return (int)((double)t * ratio); }
static inline long addr_of(const uint32_t* pt, int log_r, int r) { return ((long)pt[r >> log_r] << log_r) + (r & ((1 << log_r) - 1)); }
extern "C" {
int fwd_run_end_of(int t, double ratio, double inv, int limit, int log_r, int ahead, int T) { return dynband::fwd_run_end(t, ratio, inv, limit, log_r, ahead, T); }
int fwd_address_run_end_of(int t, int limit, int log_r, int ahead, int T) { return dynband::fwd_address_run_end(t, limit, log_r, ahead, T); }
int bwd_run_first_of(int t, double ratio, double inv, int floor_row, int log_r) { return dynband::bwd_run_first(t, ratio, inv, floor_row, log_r); }

// The forward sweep's walk. Returns 0, or a code (1000 * kind + ...) and the offending row in *bad.
//   out[r] / fetch[r]: how often row r was written / the fetch of row r was issued (the caller checks the tiling)
long walk_forward(int T, int N, int log_r, int ahead, const uint32_t* pt, int* out_cnt, int* runs, long* bad) {
  const double ratio = (double)N / (double)T, inv = 1.0 / ratio;
  long n_runs = 0;
  for (int tb = 1; tb < T; tb += 64) {
    const int tend = tb + (64 < T - tb ? 64 : T - tb);
    int t = tb;
    while (t < tend) {
      const int te = dynband::fwd_run_end(t, ratio, inv, tend, log_r, ahead, T);
      if (te <= t || te > tend) { *bad = t; return 1; }
      // the scan: the run ends in front of the first row at which anything the run holds constant changes
      int want = t + 1;
      for (; want < tend; ++want) {
        const int r = want;
        if (mid(r + 1, ratio) != mid(t + 1, ratio)) break;            // the window of row r + 1 is the run's
        if ((r >> log_r) != (t >> log_r)) break;                      // the written row's page
        const int d0 = t + ahead, d = r + ahead;
        if ((d0 < T) != (d < T)) break;                               // one side of the clamp
        if (d < T && (d >> log_r) != (d0 >> log_r)) break;            // the fetched row's page
      }
      if (te != want) { *bad = t; return 2; }
      // running addresses against the looked-up ones
      long a_out = addr_of(pt, log_r, t);
      long a_fetch = addr_of(pt, log_r, t + ahead < T ? t + ahead : T);
      const long step = dynband::fwd_fetch_advances(t, ahead, T) ? 1 : 0;
      for (int r = t; r < te; ++r) {
        if (a_out != addr_of(pt, log_r, r)) { *bad = r; return 3; }
        if (a_fetch != addr_of(pt, log_r, r + ahead < T ? r + ahead : T)) { *bad = r; return 4; }
        ++out_cnt[r];
        a_out += 1;
        a_fetch += step;
      }
      t = te;
      ++n_runs;
    }
  }
  *runs = (int)n_runs;
  return 0;
}

// The backward sweep's walk: blocks of 64 rows down from row T - 2, one cursor.
long walk_backward(int T, int N, int log_r, const uint32_t* pt, int* out_cnt, long* bad) {
  const double ratio = (double)N / (double)T, inv = 1.0 / ratio;
  for (int thi = T - 2; thi >= 0; thi -= 64) {
    const int tlo = thi - 63 > 0 ? thi - 63 : 0;
    int t = thi;
    while (t >= tlo) {
      const int tq = dynband::bwd_run_first(t, ratio, inv, tlo, log_r);
      if (tq > t || tq < tlo) { *bad = t; return 1; }
      int want = t;
      while (want > tlo && mid(want - 1, ratio) == mid(t, ratio) && ((want - 1) >> log_r) == (t >> log_r)) --want;
      if (tq != want) { *bad = t; return 2; }
      long a = addr_of(pt, log_r, t);
      for (int r = t; r >= tq; --r) {
        if (a != addr_of(pt, log_r, r)) { *bad = r; return 3; }
        ++out_cnt[r];
        a -= 1;
      }
      t = tq - 1;
    }
  }
  return 0;
}
}
''' % ROOT

ip = C.POINTER(C.c_int)
u32p = C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("rowruns")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    L.fwd_run_end_of.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int]
    L.fwd_address_run_end_of.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.bwd_run_first_of.argtypes = [C.c_int, C.c_double, C.c_double, C.c_int, C.c_int]
    L.walk_forward.restype = C.c_long
    L.walk_forward.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, u32p, ip, ip, C.POINTER(C.c_long)]
    L.walk_backward.restype = C.c_long
    L.walk_backward.argtypes = [C.c_int, C.c_int, C.c_int, u32p, ip, C.POINTER(C.c_long)]
    return L


def _page_table(rng, T, log_r):
    """Page numbers of rows 0 .. T, scattered: consecutive pages of a read are not neighbours in the pool."""
    n_pages = (T >> log_r) + 1
    return np.ascontiguousarray(rng.permutation(4 * n_pages + 7)[:n_pages], dtype=np.uint32)


def _walk_both(lib, rng, T, N, log_r):
    pt = _page_table(rng, T, log_r)
    bad, runs = C.c_long(-1), C.c_int(0)
    cnt = np.zeros(T + 1, dtype=np.int32)
    rc = lib.walk_forward(T, N, log_r, AHEAD, pt.ctypes.data_as(u32p), cnt.ctypes.data_as(ip), C.byref(runs), C.byref(bad))
    assert rc == 0, ("forward", rc, bad.value, T, N, log_r)
    assert cnt[0] == 0 and cnt[T] == 0 and (cnt[1:T] == 1).all(), ("forward rows 1 .. T-1 once each", T, N, log_r)
    cnt[:] = 0
    rc = lib.walk_backward(T, N, log_r, pt.ctypes.data_as(u32p), cnt.ctypes.data_as(ip), C.byref(bad))
    assert rc == 0, ("backward", rc, bad.value, T, N, log_r)
    assert (cnt[:T - 1] == 1).all() and cnt[T - 1] == 0 and cnt[T] == 0, ("backward rows T-2 .. 0 once each", T, N, log_r)
    return runs.value


def _ratios(T):
    """N for a read of T rows across the band's range: N / T = 1, just below, 2/3, 1/2, 1/3, ~0.1 (and its neighbours), 1/64,
    one k-mer, two."""
    ns = {T, T - 1, 2 * T // 3, T // 2, T // 3, T // 10, T // 10 + 1, T // 64, 1, 2}
    return sorted(n for n in ns if 1 <= n <= T)


@pytest.mark.parametrize("log_r", range(9))
def test_runs_equal_the_scan_small_reads_every_T(lib, log_r):
    """Every T from the minimum (2 rows) to 200, then a stride to a few thousand: every ratio class, a scattered page table."""
    rng = np.random.default_rng(1000 + log_r)
    for T in list(range(2, 201)) + list(range(201, 4100, 97)):
        for N in _ratios(T):
            _walk_both(lib, rng, T, N, log_r)


@pytest.mark.parametrize("log_r", range(9))
def test_last_rows_on_and_next_to_a_page_boundary(lib, log_r):
    """T - 1 and T - 1 - RING_D landing on a page's first row, one before and one after: the clamp and the last page crossing
    of either cursor fall together or one row apart."""
    rng = np.random.default_rng(2000 + log_r)
    R = 1 << log_r
    for k in (1, 2, 3, 7, 16, 40):
        for delta in (-1, 0, 1):
            for T in (k * R + delta + 1, k * R + delta + 1 + RING_D):
                if T < 2:
                    continue
                for N in _ratios(T):
                    _walk_both(lib, rng, T, N, log_r)


def test_no_run_spans_a_page_crossing_or_the_clamp(lib):
    """The property itself, from Python, on reads small enough to restate: inside [t, end) both cursors keep their page and
    their side of the clamp -- and end is as far as that holds (or the limit)."""
    for log_r in range(9):
        R = 1 << log_r
        for T in (2, 3, 6, 7, 8, 9, 33, 64, 65, 66, 70, 127, 128, 129, 133, 134, 257, 261, 262, 600):
            for t in range(1, T):
                limit = min(T, t + 64)
                end = lib.fwd_address_run_end_of(t, limit, log_r, AHEAD, T)
                assert t < end <= limit
                rows = range(t, end)
                assert len({r // R for r in rows}) == 1
                assert len({r + AHEAD < T for r in rows}) == 1
                if t + AHEAD < T:
                    assert len({(r + AHEAD) // R for r in rows}) == 1
                if end < limit:   # maximal: the next row breaks one of them
                    r = end
                    assert r // R != t // R or (r + AHEAD < T) != (t + AHEAD < T) or (t + AHEAD < T and (r + AHEAD) // R != (t + AHEAD) // R)


def test_one_page_read_has_the_band_runs_only(lib):
    """Pages larger than the read: the address runs add the clamp's break and nothing else."""
    rng = np.random.default_rng(7)
    T, N = 3000, 300
    ratio = float(N) / float(T)
    for t in range(1, T - AHEAD):
        limit = min(T, t + 64)
        # rows t .. want-1 share the window of row t + 1; the fetch reaches row T at t = T - AHEAD
        want = next((r for r in range(t + 1, limit) if int(float(r + 1) * ratio) != int(float(t + 1) * ratio)), limit)
        got = lib.fwd_run_end_of(t, ratio, 1.0 / ratio, limit, 12, AHEAD, T)
        assert got == min(want, T - AHEAD), t
    assert _walk_both(lib, rng, T, N, 12) > 0
