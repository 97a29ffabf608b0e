"""The rescale kernels (csrc/rescale.hip: k_rescale_init, k_rescale_fit, k_rescale_apply) pinned bit for bit at kernel level.

tests/test_gpu_rescale.py reaches them only through whole alignments, where the row count, the segment lengths and the fit's
values are whatever the aligner makes of a read. Here tests/device_math/rescale.hip, compiled with the product's flags, hands
launch_rescale_init and launch_rescale_pass borders, model means, signals and entry states built on the host, and the state
of every read (A, B, applied, frozen, fitted), the row means of every read that reached the fit and the WHOLE signal array
afterwards are compared with the restatement (tests/rescale_chain.py: chunked_sum, segment_means, fit, rescale_pass).

Not GPU-marked: that the harness compiles, that the edge constructions land on the stated side of each guard in the
restatement, and that the 65 541-descriptor batch can tell a launch slice handed the wrong descriptors from the right one.

No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rescale_chain as rc
from conftest import ROOT
from dynamont_amd import _native

gpu = pytest.mark.gpu

RS = np.dtype([("A", "<f8"), ("B", "<f8"), ("applied", "<i4"), ("frozen", "<i4"), ("fitted", "<i4"), ("pad", "<i4")])  # RescaleState
FAILED = 3
POISON = 0xA5
POISON_U64 = np.uint64(0xA5A5A5A5A5A5A5A5)
GUARD = 64                # tests/device_math/rescale.hip, RSH_GUARD
SLICE = 65535             # the most reads one launch of k_rescale_apply takes (gridDim.y)
TAIL = 6
ROW_COUNTS = (15, 16, 17, 63, 64, 65)
LONG_ROW_COUNTS = (16384, 16400)          # 256 chunks of 64 rows fill the one pass of rs_row_sum; 257 need a second
SEGMENT_LENGTHS = (2, 64, 65, 256, 257, 16384, 16385, 20000)
FRESH = (0.0, 1.0, 0, 0, 0)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the reads ---------------------------------------------------------------------------------------------------------------
def read(name, lens, m, x, state=FRESH, status=0, x0=None, expect=None):
    """lens: samples per row; m: model mean per row; x: the signal of the pass; x0: the preprocessed signal (default: x)"""
    lens = np.asarray(lens, dtype=np.int64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert len(m) == len(lens) and len(x) == lens.sum() and lens.min() >= 1
    return dict(name=name, sp=np.cumsum(lens) - lens, m=np.ascontiguousarray(m, dtype=np.float64), x=x,
                x0=x if x0 is None else np.ascontiguousarray(x0, dtype=np.float64), state=state, status=status, expect=expect)


def line_read(name, rng, lens, state=FRESH, status=0, b=1.1, a=-0.2, noise=0.05):
    """a read whose levels follow y = b m + a: the fit passes its guards"""
    n = len(lens)
    m = rng.uniform(-2.0, 2.0, n)
    x0 = np.repeat(b * m + a, lens) + noise * rng.standard_normal(int(np.sum(lens)))
    A, B = state[0], state[1]
    return read(name, lens, m, (x0 - A) / B if state[2] else x0, state, status, x0=x0)


def edge_read(name, bb, c, bump=0.0, expect=None):
    """16 rows of two equal samples: m = (-1, 1, 0, ...), levels (c - bb, c + bb, c + bump, c, ...). Every sum of the fit is
    exact for the dyadic values used below: mbar = 0, Sxx = 2, Sxy = 2 bb, b = bb, a = ybar = c + bump / 16."""
    m = np.zeros(16)
    m[0], m[1] = -1.0, 1.0
    y = np.full(16, np.float64(c))
    y[0], y[1], y[2] = c - bb, c + bb, c + bump
    return read(name, np.full(16, 2), m, np.repeat(y, 2), expect=expect)


def above(v):
    return np.nextafter(np.float64(v), np.float64(np.inf))


def below(v):
    return np.nextafter(np.float64(v), np.float64(-np.inf))


def edge_reads():
    """(b, a, applied) the restatement must give is in `expect`"""
    return [
        edge_read("b=0.5", 0.5, 0.25, expect=(0.5, 0.25, True)),
        edge_read("b<0.5", below(0.5), 0.0, expect=(below(0.5), 0.0, False)),
        edge_read("b=2", 2.0, 0.0, expect=(2.0, 0.0, True)),
        edge_read("b>2", above(2.0), 0.0, expect=(above(2.0), 0.0, False)),
        edge_read("a=2", 1.0, 2.0, expect=(1.0, 2.0, True)),
        edge_read("a>2", 1.0, 2.0, bump=2.0 ** -47, expect=(1.0, above(2.0), False)),
        edge_read("a=-2", 1.0, -2.0, expect=(1.0, -2.0, True)),
        edge_read("a<-2", 1.0, -2.0, bump=-2.0 ** -47, expect=(1.0, below(-2.0), False)),
    ]


def main_reads():
    rng = np.random.default_rng(20261019)
    reads = []
    for n in ROW_COUNTS:
        reads.append(line_read("rows/%d" % n, rng, rng.integers(1, 9, n)))
    for n in LONG_ROW_COUNTS:
        reads.append(line_read("rows/%d" % n, rng, np.full(n, 2)))
    lens = rng.integers(1, 9, 20)
    lens[[1, 3, 5, 7, 9, 11, 13, 15]] = SEGMENT_LENGTHS                      # 53 000 samples: > 16 x 256, k_rescale_apply strides
    reads.append(line_read("segment_lengths", rng, lens))
    lens = rng.integers(1, 9, 18)
    lens[[0, 17]] = 300, 257                                                  # stalls as the first and the last row
    reads.append(line_read("stall_first_and_last", rng, lens))
    reads += edge_reads()
    reads.append(read("sxx=0", np.full(16, 3), np.full(16, 0.75), rng.normal(0, 1, 48), expect=(None, None, False)))
    reads.append(read("equal_means_0.1", np.full(17, 2), np.full(17, 0.1), rng.normal(0, 1, 34)))
    r = line_read("nan_sample", rng, rng.integers(2, 6, 20))
    x = r["x"].copy()
    x[7] = np.nan
    reads.append(read("nan_sample", np.diff(np.append(r["sp"], len(x))), r["m"], x))
    reads.append(line_read("frozen_on_entry", rng, rng.integers(1, 9, 30), state=(0.3, 1.2, 1, 1, 0)))
    reads.append(line_read("failed", rng, rng.integers(1, 9, 30), status=FAILED))
    reads.append(line_read("failed_was_fitted", rng, rng.integers(1, 9, 30), state=(0.3, 1.2, 1, 0, 1), status=FAILED))
    reads.append(line_read("composition", rng, rng.integers(1, 9, 40), state=(0.3, 1.2, 1, 0, 1), b=1.2, a=0.3))
    reads.append(line_read("slope_refused", rng, rng.integers(1, 9, 40), b=2.5))
    reads.append(line_read("shift_refused", rng, rng.integers(1, 9, 40), a=2.5))
    reads.append(line_read("one_row", rng, [5]))
    for k in range(12):
        reads.append(line_read("small/%d" % k, rng, rng.integers(1, 9, int(rng.integers(10, 40))), status=FAILED if k == 5 else 0))
    return reads


class Batch:
    """reads in INPUT order; the pools (signal, model means, rows) in input order, the descriptors in `order`"""

    def __init__(self, S, nrow, status, order, sig, sig0, par_mean, segrow, rs):
        S, nrow = np.asarray(S, dtype=np.int64), np.asarray(nrow, dtype=np.int64)
        self.n = len(S)
        self.sig_start, self.row_start = np.cumsum(S) - S, np.cumsum(nrow) - nrow
        self.S, self.nrow = S, nrow
        order = np.asarray(order, dtype=np.int64)
        self.read = order.astype(np.uint32)
        self.T, self.N = (S[order] + 1).astype(np.uint32), (nrow[order] + 1).astype(np.uint32)
        self.sig_off = self.sig_start[order].astype(np.uint64)
        self.seg_off = self.row_start[order].astype(np.uint64)
        self.par_off = self.seg_off.copy()                                     # one model mean per row
        self.status = np.ascontiguousarray(status, dtype=np.int32)
        self.sig, self.sig0, self.par_mean, self.segrow, self.rs = sig, sig0, par_mean, np.ascontiguousarray(segrow, dtype=np.uint32), rs
        for a in (self.read, self.T, self.N, self.sig_off, self.seg_off, self.par_off, self.status, sig, sig0, par_mean, self.segrow, rs):
            a.setflags(write=False)


def batch_of(reads, order):
    rs = np.zeros(len(reads), dtype=RS)
    for i, r in enumerate(reads):
        rs[i] = tuple(r["state"]) + (0,)
    return Batch([len(r["x"]) for r in reads], [len(r["m"]) for r in reads], [r["status"] for r in reads], order,
                 np.concatenate([r["x"] for r in reads]), np.concatenate([r["x0"] for r in reads]),
                 np.concatenate([r["m"] for r in reads]), np.concatenate([r["sp"] + 1 for r in reads]), rs)


def expected(b, fit_reads, apply_descs=None):
    """(rs, y, sig) as the pass must leave them: y and the guards hold the poison wherever nothing may be written. fit_reads:
    the reads that get as far as the row means (the others -- failed, frozen, fewer than 16 rows -- are restated for the whole
    batch at once). apply_descs: the descriptors k_rescale_apply is handed (default: all of them)."""
    rs = b.rs.copy()
    out = (b.status != 0) | (rs["frozen"] != 0) | (b.nrow < rc.MIN_ROWS)
    assert np.array_equal(np.flatnonzero(~out), np.sort(fit_reads))
    rs["frozen"][out], rs["fitted"][out] = 1, 0
    y = np.full(int(b.nrow.sum()) + GUARD, POISON_U64).view(np.float64)
    sig = np.concatenate([b.sig, np.full(GUARD, POISON_U64).view(np.float64)])
    applied_to = np.ones(b.n, dtype=bool)
    if apply_descs is not None:
        applied_to[:] = False
        applied_to[b.read[apply_descs]] = True
    for i in fit_reads:
        s0, r0, S, n = int(b.sig_start[i]), int(b.row_start[i]), int(b.S[i]), int(b.nrow[i])
        st, yi, x = rc.rescale_pass(b.sig[s0:s0 + S], b.sig0[s0:s0 + S], b.segrow[r0:r0 + n].astype(np.int64) - 1, b.par_mean[r0:r0 + n],
                                    tuple(b.rs[i])[:5])
        rs[i] = st + (0,)
        y[r0:r0 + n] = yi
        if applied_to[i]:
            sig[s0:s0 + S] = x
    return rs, y, sig


@pytest.fixture(scope="module")
def main():
    reads = main_reads()
    rng = np.random.default_rng(5)
    order = rng.permutation(len(reads))
    order = order[np.argsort(-np.array([len(reads[i]["x"]) for i in order]), kind="stable")]   # launch.cpp: long reads first
    b = batch_of(reads, order)
    b.reads = reads
    b.index = {r["name"]: i for i, r in enumerate(reads)}
    assert len(b.index) == len(reads)
    return b


@pytest.fixture(scope="module")
def main_want(main):
    fit_reads = [i for i, r in enumerate(main.reads) if r["status"] == 0 and not r["state"][3] and len(r["m"]) >= rc.MIN_ROWS]
    return expected(main, fit_reads)


def build_sliced():
    """65 541 descriptors, most of them failed reads of T = 3; ok reads of 16 two-sample rows: five in the first slice, and
    descriptors 65 535 .. 65 540. Built without a loop over the reads."""
    rng = np.random.default_rng(48)
    n = SLICE + TAIL
    ok = np.sort(rng.choice(np.arange(100, n - 100), 5 + TAIL, replace=False))   # read indices, scattered over the input order
    tail = ok[rng.permutation(len(ok))[:TAIL]]
    nrow = np.ones(n, dtype=np.int64)
    nrow[ok] = 16
    S = 2 * nrow
    status = np.full(n, FAILED, dtype=np.int32)
    status[ok] = 0
    status[rng.choice(np.setdiff1d(np.arange(n), ok), 200, replace=False)] = 0       # ok reads of one row: refused, not failed
    rest = np.setdiff1d(np.arange(n), tail)
    order = np.concatenate([rest[np.argsort(-nrow[rest], kind="stable")], tail])
    row_read = np.repeat(np.arange(n), nrow)
    row_in_read = np.arange(int(nrow.sum())) - np.repeat(np.cumsum(nrow) - nrow, nrow)
    par_mean = rng.uniform(-2.0, 2.0, len(row_read))
    level = (0.9 + 0.3 * rng.random(n))[row_read] * par_mean + (0.4 * rng.random(n) - 0.2)[row_read]
    sig = np.repeat(level, 2) + 0.05 * rng.standard_normal(2 * len(level))
    rs = np.zeros(n, dtype=RS)
    rs["B"] = 1.0
    b = Batch(S, nrow, status, order, sig, sig.copy(), par_mean, 2 * row_in_read + 1, rs)
    b.ok16, b.tail = ok, tail
    return b


@pytest.fixture(scope="module")
def sliced():
    return build_sliced()


@pytest.fixture(scope="module")
def sliced_want(sliced):
    return expected(sliced, sliced.ok16)


# ---- the harness -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness_so(tmp_path_factory):
    """tests/device_math/rescale.hip -> a shared library, with the flags of every translation unit of the product"""
    so = tmp_path_factory.mktemp("rescale") / "librescalek.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/rescale.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(so)


@pytest.fixture(scope="module")
def lib(harness_so, native_lib):
    h = C.CDLL(harness_so)
    h.rs_run.restype = C.c_int
    return h


def run_on_device(lib, b, max_T=0):
    """rs_run -> (rs, y, sig) with their guards; every HIP call returned hipSuccess; launch_rescale_init left A = 0, B = 1 and
    zeros in every read's state"""
    rs, rs_init = b.rs.copy(), np.zeros(b.n, dtype=RS)
    sig = np.concatenate([b.sig, np.zeros(GUARD)])
    y = np.zeros(len(b.segrow) + GUARD)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.rs_run(C.c_int(len(b.read)), p(b.sig_off), p(b.par_off), p(b.seg_off), p(b.T), p(b.N), p(b.read), C.c_int(b.n), p(b.status),
                   p(rs), p(rs_init), C.c_uint64(len(b.sig)), p(b.sig0), p(sig), C.c_uint64(len(b.par_mean)), p(b.par_mean),
                   C.c_uint64(len(b.segrow)), p(b.segrow), p(y), C.c_uint32(max_T), C.c_int(POISON), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    fresh = np.zeros(b.n, dtype=RS)
    fresh["B"] = 1.0
    assert rs_init.tobytes() == fresh.tobytes(), "launch_rescale_init"
    return rs, y, sig


def compare(b, got, want, names=None):
    """every field of every read's state, every row mean (the poison where none may be written) and the whole signal"""
    (g_rs, g_y, g_sig), (w_rs, w_y, w_sig) = got, want
    name = (lambda i: names[i]) if names else (lambda i: "read %d" % i)
    for f in RS.names:
        gf, wf = (bits(g_rs[f]), bits(w_rs[f])) if f in "AB" else (g_rs[f], w_rs[f])
        bad = np.flatnonzero(gf != wf)
        assert bad.size == 0, (f, [(name(i), g_rs[f][i], w_rs[f][i]) for i in bad[:5]])
    bad = np.flatnonzero(bits(g_y) != bits(w_y))
    rows = np.searchsorted(b.row_start, bad[:5], side="right") - 1
    assert bad.size == 0, ("y", len(bad), [(name(i), int(j - b.row_start[i]), g_y[j], w_y[j]) for i, j in zip(rows, bad[:5])])
    bad = np.flatnonzero(bits(g_sig) != bits(w_sig))
    reads = np.searchsorted(b.sig_start, bad[:5], side="right") - 1
    assert bad.size == 0, ("sig", len(bad), [(name(i), int(j - b.sig_start[i]), g_sig[j], w_sig[j]) for i, j in zip(reads, bad[:5])])


# ---- not GPU-marked ----------------------------------------------------------------------------------------------------------
def test_harness_compiles_with_the_products_flags(harness_so):
    assert os.path.getsize(harness_so) > 0


def test_edge_constructions_land_on_their_side_of_each_guard():
    """the restatement gives exactly b == 0.5, b == 2, |a| == 2 (applied) and the next double beyond each (refused)"""
    seen = set()
    for r in edge_reads():
        y = rc.segment_means(r["x"], r["sp"])
        a, b, ok = rc.fit(r["m"], y)
        wb, wa, wok = r["expect"]
        assert bits(b)[0] == bits(wb)[0] and bits(a)[0] == bits(wa)[0] and ok == wok, (r["name"], float(a).hex(), float(b).hex(), ok)
        seen.add((float(b), float(abs(a)), ok))
    assert {(0.5, 0.25, True), (2.0, 0.0, True), (1.0, 2.0, True)} <= seen
    assert {(float(below(0.5)), 0.0, False), (float(above(2.0)), 0.0, False), (1.0, float(above(2.0)), False)} <= seen
    assert below(0.5) < 0.5 < 2.0 < above(2.0)


def test_main_batch_holds_what_it_is_named_for(main, main_want):
    rs, y, sig = main_want
    i = main.index
    nrow = {int(v) for v in main.nrow}
    assert set(ROW_COUNTS) | set(LONG_ROW_COUNTS) <= nrow and 1 in nrow
    for n in ROW_COUNTS + LONG_ROW_COUNTS:                                    # 15 rows: refused; from 16 on: fitted
        k = i["rows/%d" % n]
        assert (rs["fitted"][k], rs["frozen"][k], rs["applied"][k]) == ((1, 0, 1) if n >= 16 else (0, 1, 0)), n
    assert [(n + rc.CHUNK - 1) // rc.CHUNK for n in LONG_ROW_COUNTS] == [256, 257]   # the last chunk of pass one; pass two
    for n in LONG_ROW_COUNTS:
        assert main.S[i["rows/%d" % n]] == 2 * n
    k = i["segment_lengths"]
    lens = np.diff(np.append(main.segrow[int(main.row_start[k]):int(main.row_start[k]) + int(main.nrow[k])].astype(np.int64) - 1, main.S[k]))
    assert set(SEGMENT_LENGTHS) <= set(lens.tolist()) and main.S[k] > 16 * 256 and rs["fitted"][k] == 1
    k = i["sxx=0"]
    m = main.par_mean[int(main.row_start[k]):int(main.row_start[k]) + 16]
    assert rc.chunked_sum((m - rc.chunked_sum(m) / 16.0) ** 2) == 0.0 and rs["frozen"][k] == 1 and rs["fitted"][k] == 0
    assert np.isnan(sig[int(main.sig_start[i["nan_sample"]]) + 7]) and rs["frozen"][i["nan_sample"]] == 1
    assert np.isnan(y[int(main.row_start[i["nan_sample"]]):int(main.row_start[i["nan_sample"]]) + 20]).sum() == 1
    for name in ("frozen_on_entry", "failed", "failed_was_fitted", "one_row", "rows/15"):   # no row mean, the signal as handed in
        k = i[name]
        assert (bits(y[int(main.row_start[k]):int(main.row_start[k]) + int(main.nrow[k])]) == POISON_U64).all(), name
        assert rs["frozen"][k] == 1 and rs["fitted"][k] == 0
        assert (rs["A"][k], rs["B"][k], rs["applied"][k]) == (main.rs["A"][k], main.rs["B"][k], main.rs["applied"][k])
    k = i["composition"]
    assert rs["applied"][k] == 2 and rs["fitted"][k] == 1 and abs(rs["A"][k] - 0.3) < 0.1 and abs(rs["B"][k] - 1.2) < 0.1
    assert bits(rs["A"][k])[0] != bits(0.3)[0] and bits(rs["B"][k])[0] != bits(1.2)[0]
    assert rs["frozen"][i["slope_refused"]] == 1 and rs["frozen"][i["shift_refused"]] == 1
    fitted = np.flatnonzero(rs["fitted"] == 1)
    changed = np.array([(bits(sig[int(main.sig_start[k]):int(main.sig_start[k]) + int(main.S[k])])
                         != bits(main.sig[int(main.sig_start[k]):int(main.sig_start[k]) + int(main.S[k])])).any() for k in range(main.n)])
    assert np.array_equal(np.flatnonzero(changed), fitted) and len(fitted) >= 20 and (rs["fitted"] == 0).sum() >= 14
    assert (main.read != np.arange(main.n)).sum() > main.n // 2               # the descriptors are not in input order
    assert main.T.max() > 16 * 256 and (main.T.max() + 255) // 256 >= 16      # gx = 16; max_T = 200 gives gx = 1


def test_inputs_tell_a_wrong_slice_apart(sliced, sliced_want):
    """A second launch of k_rescale_apply that is handed the first descriptors again (descs in place of descs + r0) leaves the
    signal of descriptors 65 535 .. 65 540 as it was: every one of them is an ok read whose fit is applied."""
    s = sliced
    assert len(s.read) == SLICE + TAIL and np.array_equal(np.sort(s.read[SLICE:]), np.sort(s.tail))
    assert (s.status != 0).sum() > 65000 and (s.T[s.status[s.read] != 0] == 3).all()
    rs, _, sig = sliced_want
    assert (rs["fitted"][s.ok16] == 1).all() and (rs["fitted"] == 1).sum() == len(s.ok16) == 5 + TAIL
    assert np.isin(s.read[:SLICE], s.ok16).sum() == 5
    _, _, other = expected(s, s.ok16, apply_descs=np.concatenate([np.arange(SLICE), np.arange(TAIL)]))
    for i in s.tail:
        a = slice(int(s.sig_start[i]), int(s.sig_start[i]) + 32)
        assert (bits(other[a]) != bits(sig[a])).all() and (bits(other[a]) == bits(s.sig[a])).all(), i


# ---- on the device -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("max_T", [0, 200], ids=["gx=16", "gx=1"])
def test_pass_bit_for_bit(lib, main, main_want, max_T):
    """Row counts 15 .. 17, 63 .. 65, 16 384 and 16 400; segments of 2 .. 20 000 samples; the guards at b = 0.5, b = 2, |a| = 2
    and one double beyond; Sxx = 0; a NaN sample; a frozen, a failed and a composed entry state. The grid of k_rescale_apply
    sized by the longest read (16 workgroups per read) and by max_T = 200 (one: every read strides)."""
    names = [r["name"] for r in main.reads]
    compare(main, run_on_device(lib, main, max_T), main_want, names)


@gpu
def test_more_reads_than_one_launch_slice(lib, sliced, sliced_want):
    """65 541 descriptors: k_rescale_apply runs a second launch over descriptors 65 535 .. 65 540"""
    compare(sliced, run_on_device(lib, sliced), sliced_want)
