"""CPU: the host-only rules of the launch path (dynamont_amd/csrc/launch_plan.hpp) compiled with g++ behind an extern "C" shim,
each against its restatement in Python: what a read costs and the order of a queue, the length re-sort, a read's pages and the
pages that keep every wave busy, the posterior layout with its DYN_FORCE_LAYOUT override, and every field of a descriptor.

The classic launch, the resident session and the guide pre-pass all take these rules from the header, so what is pinned here is
pinned for the three of them."""
import ctypes as C
import subprocess

import pytest

from conftest import ROOT

SRC = r'''
#include "%s/dynamont_amd/csrc/launch_plan.hpp"
// the fields of dynk::ReadDesc (nt_kernels.hpp), by name: make_desc is a template over the descriptor type
struct Desc {
  uint64_t sig_off, par_off, path_off, seg_off;
  uint32_t T, N, bw, read;
  double ratio;
  uint32_t first_page, n_pages, flags, strict_rows;
};
extern "C" {
uint64_t lp_cost_rows(uint64_t T, uint32_t strict_rows) { return dynplan::cost_rows(T, strict_rows); }
void lp_cost_order(uint32_t* order, uint64_t n, const uint64_t* S, const uint32_t* strict_rows) {
  std::vector<uint32_t> o(order, order + n);
  dynplan::cost_order(o, [&](uint32_t i) { return S[i]; }, strict_rows);
  std::copy(o.begin(), o.end(), order);
}
void lp_length_order(uint32_t* order, uint64_t n, const uint64_t* S) {
  std::vector<uint32_t> o(order, order + n);
  dynplan::length_order(o, [&](uint32_t i) { return S[i]; });
  std::copy(o.begin(), o.end(), order);
}
void lp_make_desc(Desc* out, uint32_t read, uint64_t S, uint64_t kc, uint64_t half_band, uint64_t sig_off, uint64_t par_off,
                  uint64_t seg_off, uint64_t path_off, uint32_t strict_rows) {
  *out = dynplan::make_desc<Desc>(read, S, kc, half_band, sig_off, par_off, seg_off, path_off, strict_rows);
}
uint32_t lp_pages_of(uint64_t S, int log_r) { return dynplan::pages_of(S, log_r); }
uint64_t lp_pages_wanted(const uint32_t* pages, uint64_t n, uint64_t n_slots) {
  std::vector<uint32_t> pg(pages, pages + n);
  return dynplan::pages_wanted(pg, (size_t)n_slots);
}
int lp_choose_lpe_layout(uint64_t budget, uint64_t wanted, uint64_t page_rows) { return dynplan::choose_lpe_layout(budget, wanted, page_rows) ? 1 : 0; }
uint64_t lp_row_sep() { return dynplan::row_sep; }
uint64_t lp_row_inp() { return dynplan::row_inp; }
}
''' % ROOT

ALL = 0xFFFFFFFF
NO_PAGE = 0xFFFFFFFF
READ_STRICT, READ_STRICT_START = 1, 2
# bytes of a lattice row: 448 band slots of 8 B (+ 4 B of float LPE where it is kept apart) and the row's 64-byte record
ROW_SEP, ROW_INP = 448 * 12 + 64, 448 * 8 + 64


class Desc(C.Structure):
    _fields_ = [("sig_off", C.c_uint64), ("par_off", C.c_uint64), ("path_off", C.c_uint64), ("seg_off", C.c_uint64),
                ("T", C.c_uint32), ("N", C.c_uint32), ("bw", C.c_uint32), ("read", C.c_uint32), ("ratio", C.c_double),
                ("first_page", C.c_uint32), ("n_pages", C.c_uint32), ("flags", C.c_uint32), ("strict_rows", C.c_uint32)]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("launchplan")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.lp_cost_rows.restype = C.c_uint64
    L.lp_cost_rows.argtypes = [C.c_uint64, C.c_uint32]
    L.lp_cost_order.restype = None
    L.lp_cost_order.argtypes = [u32p, C.c_uint64, u64p, u32p]
    L.lp_length_order.restype = None
    L.lp_length_order.argtypes = [u32p, C.c_uint64, u64p]
    L.lp_make_desc.restype = None
    L.lp_make_desc.argtypes = [C.POINTER(Desc), C.c_uint32] + [C.c_uint64] * 7 + [C.c_uint32]
    L.lp_pages_of.restype = C.c_uint32
    L.lp_pages_of.argtypes = [C.c_uint64, C.c_int]
    L.lp_pages_wanted.restype = C.c_uint64
    L.lp_pages_wanted.argtypes = [u32p, C.c_uint64, C.c_uint64]
    L.lp_choose_lpe_layout.restype = C.c_int
    L.lp_choose_lpe_layout.argtypes = [C.c_uint64] * 3
    L.lp_row_sep.restype = L.lp_row_inp.restype = C.c_uint64
    return L


def _cost(T, strict_rows):
    """A certified backward row costs 1.3, a certified forward row 1.4 default rows; 0.4 / 0.6 of a read are the two sweeps:
    0.4 T x 1.3 + 0.6 (T + 0.4 fr) = 1.12 T + 0.24 fr, fr the certified forward rows; in integers, rounded down."""
    if strict_rows == 0:
        return T
    return (112 * T + 24 * min(T, strict_rows)) // 100


# 12 reads, S in 50 .. 3000, equal lengths among them; strict rows 0, a mid-read value, every row
S12 = [3000, 74, 1200, 1200, 2999, 800, 1200, 3000, 101, 800, 2500, 50]
STRICT12 = [0, ALL, 0, 600, 0, ALL, 0, 1, 0, ALL, 2500, 0]


def _arr(t, v):
    return (t * len(v))(*v)


def test_cost_of_a_read(lib):
    for T in (1, 2, 51, 801, 1201, 3001, 200_001):
        for sr in (0, 1, T // 2, T - 1, T, T + 1, ALL):
            assert lib.lp_cost_rows(T, sr) == _cost(T, sr), (T, sr)
    # a default read costs its rows; a read certified throughout (1.12 + 0.24) T, rounded down
    assert lib.lp_cost_rows(1000, 0) == 1000 and lib.lp_cost_rows(1000, ALL) == 1360 and lib.lp_cost_rows(1000, 500) == 1240


def test_cost_order_is_exact_and_stable(lib):
    n = len(S12)
    cost = [_cost(S12[i] + 1, STRICT12[i]) for i in range(n)]
    # (the case holds ties of three kinds: equal plain lengths, equal strict reads, and a strict read against a longer plain one of its cost)
    assert cost[2] == cost[6] and cost[5] == cost[9] and cost[1] == cost[8] == 102
    want = sorted(range(n), key=lambda i: -cost[i])          # Python's sort is stable: ties keep their input order
    order = _arr(C.c_uint32, list(range(n)))
    lib.lp_cost_order(order, n, _arr(C.c_uint64, S12), _arr(C.c_uint32, STRICT12))
    assert list(order) == want
    for x, y in zip(want, want[1:]):
        assert cost[x] > cost[y] or (cost[x] == cost[y] and x < y)
    # stability is about the order that comes IN: reversed input, ties reversed
    rev = list(range(n))[::-1]
    order = _arr(C.c_uint32, rev)
    lib.lp_cost_order(order, n, _arr(C.c_uint64, S12), _arr(C.c_uint32, STRICT12))
    assert list(order) == sorted(rev, key=lambda i: -cost[i])
    # without strict reads the cost order is the length order
    order = _arr(C.c_uint32, list(range(n)))
    lib.lp_cost_order(order, n, _arr(C.c_uint64, S12), _arr(C.c_uint32, [0] * n))
    assert list(order) == sorted(range(n), key=lambda i: -S12[i])


def test_length_resort(lib):
    """What a starved launch with strict reads and a paged session go back to: longest first whatever the strict rows, ties in
    the order they come in -- here the cost order."""
    n = len(S12)
    cost_order = sorted(range(n), key=lambda i: -_cost(S12[i] + 1, STRICT12[i]))
    order = _arr(C.c_uint32, cost_order)
    lib.lp_length_order(order, n, _arr(C.c_uint64, S12))
    assert list(order) == sorted(cost_order, key=lambda i: -S12[i])
    assert [S12[i] for i in order] == sorted(S12, reverse=True)
    assert list(order) != cost_order


def _layout(budget, wanted, page_rows):
    c_sep = min(1.0, budget / (float(wanted) * page_rows * ROW_SEP + 1.0))
    c_inp = min(1.0, budget / (float(wanted) * page_rows * ROW_INP + 1.0))
    return not (c_sep < 1.0 and c_inp * 0.92 > c_sep)


def test_layout_choice_across_the_budget(lib, monkeypatch):
    """wanted x page_rows fixed, the budget swept. full_sep / full_inp: what a lattice for every wave slot takes in either layout.
      budget >= full_sep             both fit: separate (the faster sweep costs nothing)
      full_inp <= budget < full_sep  only in place fits fully: c_inp = 1, so in place iff c_sep < 0.92 -- the 0.92 threshold
                                     lies in THIS region, at budget = 0.92 full_sep (> full_inp = 0.67 full_sep)
      budget < full_inp              neither fits: c_inp / c_sep = full_sep / full_inp = 1.49 > 1 / 0.92 whatever the budget, so
                                     in place throughout (no budget of this region reaches the other side of the threshold)"""
    monkeypatch.delenv("DYN_FORCE_LAYOUT", raising=False)
    assert lib.lp_row_sep() == ROW_SEP and lib.lp_row_inp() == ROW_INP
    wanted, page_rows = 1000, 256
    full_sep, full_inp = wanted * page_rows * ROW_SEP + 1, wanted * page_rows * ROW_INP + 1
    thr = int(0.92 * full_sep)
    assert full_inp < thr < full_sep
    cases = [(full_sep * 2, True), (full_sep, True),                                   # both fit
             (full_sep - 1, True), (thr + 1000, True), (thr - 1000, False), (full_inp, False),  # only in place fits fully
             (full_inp - 1, False), (full_inp // 2, False), (full_inp // 100, False), (1, False)]  # neither fits
    for budget, separate in cases:
        assert _layout(budget, wanted, page_rows) == separate, budget
        assert lib.lp_choose_lpe_layout(budget, wanted, page_rows) == int(separate), budget
    # the sweep itself, 400 budgets from nothing to twice full_sep, and another geometry
    for w, pr in ((wanted, page_rows), (37, 1024), (1, 4)):
        top = 2 * (w * pr * ROW_SEP + 1)
        for k in range(401):
            budget = top * k // 400
            assert lib.lp_choose_lpe_layout(budget, w, pr) == int(_layout(budget, w, pr)), (w, pr, budget)
    # DYN_FORCE_LAYOUT overrides the rule in both directions: "inplace" where both fit, anything else where neither does
    monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    for budget, _ in cases:
        assert lib.lp_choose_lpe_layout(budget, wanted, page_rows) == 0
    monkeypatch.setenv("DYN_FORCE_LAYOUT", "separate")
    for budget, _ in cases:
        assert lib.lp_choose_lpe_layout(budget, wanted, page_rows) == 1
    monkeypatch.delenv("DYN_FORCE_LAYOUT")
    assert lib.lp_choose_lpe_layout(full_inp, wanted, page_rows) == 0 and lib.lp_choose_lpe_layout(full_sep, wanted, page_rows) == 1


def test_pages_of_a_read(lib):
    """Lattice rows 0 .. T = S + 1 are S + 2 rows: one page up to S = page_rows - 2, two from page_rows - 1 on."""
    for log_r in (2, 8, 10):
        pr = 1 << log_r
        assert [lib.lp_pages_of(S, log_r) for S in (pr - 2, pr - 1, pr)] == [1, 2, 2]
        assert lib.lp_pages_of(0, log_r) == 1 and lib.lp_pages_of(2 * pr - 2, log_r) == 2 and lib.lp_pages_of(2 * pr - 1, log_r) == 3
        for S in (1, 50, 255, 256, 3000, 200_000):
            assert lib.lp_pages_of(S, log_r) == -(-(S + 2) // pr)


def test_pages_that_keep_every_slot_busy(lib):
    pages = [3, 12, 1, 12, 7, 2, 9]

    def wanted(pg, n_slots):
        return lib.lp_pages_wanted(_arr(C.c_uint32, pg), len(pg), n_slots)

    assert wanted(pages, 3) == 12 + 12 + 9                    # more reads than slots: the largest lattices at once
    assert wanted(pages, 1) == 12 and wanted(pages, 0) == 0
    assert wanted(pages, 7) == sum(pages) and wanted(pages, 1024) == sum(pages)   # fewer reads than slots: all of them
    assert wanted([], 0) == 0 and wanted([], 1024) == 0       # an empty list
    for n_slots in range(9):
        assert wanted(pages, n_slots) == sum(sorted(pages, reverse=True)[:n_slots])


def _desc(lib, *args):
    d = Desc()
    lib.lp_make_desc(C.byref(d), *args)
    return {name: getattr(d, name) for name, _ in Desc._fields_}


def test_every_field_of_a_descriptor(lib):
    # read, S, kc, half_band, sig_off, par_off, seg_off, path_off, strict_rows
    queue = _desc(lib, 7, 1000, 99, 223, 11_000, 5_000, 4_900, 70_000, 0)
    assert queue == dict(sig_off=11_000, par_off=5_000, path_off=70_000, seg_off=4_900, T=1001, N=100, bw=50, read=7,
                         ratio=100.0 / 1001.0, first_page=NO_PAGE, n_pages=0, flags=0, strict_rows=0)
    strict = _desc(lib, 0, 2999, 899, 223, 0, 0, 0, 0, ALL)
    assert strict == dict(sig_off=0, par_off=0, path_off=0, seg_off=0, T=3000, N=900, bw=223, read=0, ratio=900.0 / 3000.0,
                          first_page=NO_PAGE, n_pages=0, flags=READ_STRICT, strict_rows=ALL)
    start = _desc(lib, 4_000_000_000, 50, 50, 223, 2 ** 40, 2 ** 39, 2 ** 38, 2 ** 41, 17)
    assert start == dict(sig_off=2 ** 40, par_off=2 ** 39, path_off=2 ** 41, seg_off=2 ** 38, T=51, N=51, bw=25, read=4_000_000_000,
                         ratio=1.0, first_page=NO_PAGE, n_pages=0, flags=READ_STRICT_START, strict_rows=17)


@pytest.mark.parametrize("half_band", [1, 50, 223])
def test_half_band_of_a_descriptor(lib, half_band):
    """bw = min(half_band, N / 2), N = kc + 1 (NT_aligner_api.cpp:243), at N = 1, 2, 2 half_band and 2 half_band + 1."""
    for N in (1, 2, 2 * half_band, 2 * half_band + 1):
        d = _desc(lib, 0, 5000, N - 1, half_band, 0, 0, 0, 0, 0)
        assert d["N"] == N and d["bw"] == min(half_band, N // 2), N
        assert d["ratio"] == float(N) / 5001.0
    assert _desc(lib, 0, 5000, 0, half_band, 0, 0, 0, 0, 0)["bw"] == 0
    assert _desc(lib, 0, 5000, 2 * half_band - 1, half_band, 0, 0, 0, 0, 0)["bw"] == half_band
    assert _desc(lib, 0, 5000, 2 * half_band - 2, half_band, 0, 0, 0, 0, 0)["bw"] == half_band - (1 if half_band > 0 else 0)
