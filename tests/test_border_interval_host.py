"""CPU: the host half of the per-border credible intervals (dyn_aligner_set_border_interval). The new symbols resolve and the
switch is range-checked with a message; dyn_format_csv_intervals writes the integers as integers and the floats as Python's
f"{x:.6f}", with bi == NULL the bytes of dyn_format_csv_samples, and its bound holds; the sink knows its new flag and refuses an
unknown one. The yardstick of the GPU tests (tests/border_interval_cases.py) is held against itself: every lattice column's
masses sum to 1, lo <= hi, mass 0.999 nests mass 0.5, the border confidence's window mass is consistent with the interval, the
read sets have the properties the GPU tests rely on, and five deliberately wrong versions each differ from it.
(The sink's refusal of a ticket submitted with the switch off needs a ticket, and a host-only handle creates none:
tests/test_gpu_border_interval.py holds it.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import border_interval_cases as bic
from conftest import ROOT
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd import _native as N
from dynamont_amd._dynamont import AlignBatchResult, _ptr, format_csv

pytestmark = pytest.mark.usefixtures("native_lib")

COLS = ("border_lo", "border_hi", "border_mean", "border_sd")


def test_symbols_and_constants(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_border_interval", "dyn_batch_fetch_intervals", "dyn_format_csv_intervals",
                 "dyn_format_csv_bound_intervals"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "typedef struct dyn_border_interval_out" in hdr and "DYN_ABI_VERSION 10" in hdr
    assert "DYN_BORDER_INTERVAL_MIN_MASS 0.01" in hdr and "DYN_BORDER_INTERVAL_MAX_MASS 0.999" in hdr
    # (0x40: an existing test opens sinks with 0x20 and 0x30 to see unassigned flags refused, so bit 0x20 stays unassigned)
    assert "DYN_CSV_BORDER_INTERVAL 0x40u" in hdr and N.DYN_CSV_BORDER_INTERVAL == 0x40
    assert (N.DYN_BORDER_INTERVAL_MIN_MASS, N.DYN_BORDER_INTERVAL_MAX_MASS) == (0.01, 0.999)
    assert [f[0] for f in N.DynBorderIntervalOut._fields_] == list(COLS) + ["capacity"]
    for key in COLS:
        assert getattr(AlignBatchResult(1, 1), key) is None                          # off: no columns


def test_switch_range_and_null_on_a_host_handle(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    assert al._border_interval == 0
    al.set_border_interval(0.9)
    for bad, text in ((-0.5, "-0.5"), (0.009, "0.009"), (0.9991, "0.9991"), (1.0, "1"), (2.0, "2"), (float("nan"), "-?nan"),
                      (float("inf"), "inf")):
        with pytest.raises(ValueError, match=r"dyn_aligner_set_border_interval: mass must be 0 or 0\.01 \.\. 0\.999, got " + text):
            al.set_border_interval(bad)
        assert al._border_interval == 0.9                                           # the switch stays as it was
    for ok in (0, 0.01, 0.5, 0.999, 0):
        al.set_border_interval(ok)
        assert al._border_interval == ok
    L = N.lib()
    assert L.dyn_aligner_set_border_interval(None, 0.9) == N.DYN_ERR_INVALID_ARGUMENT
    u, d = np.zeros(4, dtype=np.uint32), np.zeros(4)
    out = N.DynBorderIntervalOut(_ptr(u, N.c_u32_p), _ptr(u, N.c_u32_p), _ptr(d, N.c_double_p), _ptr(d, N.c_double_p), 4)
    assert L.dyn_batch_fetch_intervals(None, C.byref(out)) == N.DYN_ERR_INVALID_ARGUMENT
    al.close()


# ---- the formatter ---------------------------------------------------------------------------------------------------------------
SPECIAL = [0.0, 1.0, 5e-324, 0.0000005, 0.0000015, 0.9999995, 0.5, 0.1234565, 511.9999995, 512.0, 12345.6789015, 4.0e9, 1e15, 3e18]


def _fake_result(rng, n_reads, values):
    nseg = rng.integers(1, 30, n_reads)
    cap = int(nseg.sum())
    res = AlignBatchResult(n_reads, cap)
    res.seg_offsets[1:] = np.cumsum(nseg)
    res.n_segments[:] = nseg
    res.status[2] = 3   # a failed read: no rows
    res.n_segments[2] = 0
    seqs = []
    for i in range(n_reads):
        a, m = int(res.seg_offsets[i]), int(nseg[i])
        seqs.append("".join(rng.choice(list("ACGT"), m + 4)))
        res.sequence_positions[a:a + m] = np.arange(m) + 2
        res.signal_positions[a:a + m] = np.cumsum(rng.integers(1, 40, m)) - 1
        res.probabilities[a:a + m] = rng.random(m)
    res.states[:] = ord("M")
    v = np.resize(np.asarray(values, dtype=np.float64), cap)
    cols = {"border_probability": np.resize(rng.random(cap), cap), "border_window_probability": rng.random(cap),
            "border_lo": rng.integers(0, 2 ** 32, cap, dtype=np.uint64).astype(np.uint32),
            "border_hi": rng.integers(0, 2 ** 32, cap, dtype=np.uint64).astype(np.uint32),
            "border_mean": v.copy(), "border_sd": np.roll(v, 13)}
    cols["border_lo"][:3] = (0, 1, 2 ** 32 - 1)
    return res, seqs, cols


def _with_intervals(lines, res, cols, starts):
    """the rows of the formatter below with ',{lo},{hi},{mean:.6f},{sd:.6f}' appended, positions in the `start` column's unit"""
    out, k = [], 0
    for i in range(res.n):
        if res.status[i] != 0:
            continue
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        for j in range(m):
            lo, hi = int(cols["border_lo"][a + j]) + starts[i], int(cols["border_hi"][a + j]) + starts[i]
            mean = float(cols["border_mean"][a + j]) + float(starts[i])
            out.append(lines[k] + f",{lo},{hi},{mean:.6f},{cols['border_sd'][a + j]:.6f}".encode())
            k += 1
    assert k == len(lines)
    return b"".join(x + b"\n" for x in out)


@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna004", 9)])
def test_native_rows_and_bound(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    rng = np.random.default_rng(5)
    n = 12
    res, seqs, cols = _fake_result(rng, n, SPECIAL + list(rng.random(200) * 3000.0))
    rid = [f"r{i}" for i in range(n)]
    sid = [f"s{i}" for i in range(n)]
    starts = [int(x) for x in rng.integers(0, 100000, n)]
    last = [starts[i] + int(res.signal_positions[int(res.seg_offsets[i]) + max(0, int(res.n_segments[i]) - 1)]) + 50 for i in range(n)]
    L = N.lib()
    rids = (C.c_char_p * n)(*[x.encode() for x in rid])
    sids = (C.c_char_p * n)(*[x.encode() for x in sid])
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seqs])
    so, li = np.array(starts, dtype=np.int64), np.array(last, dtype=np.int64)
    bd = N.DynBorderOut(_ptr(cols["border_probability"], N.c_double_p), _ptr(cols["border_window_probability"], N.c_double_p), res.cap)
    bi = N.DynBorderIntervalOut(_ptr(cols["border_lo"], N.c_u32_p), _ptr(cols["border_hi"], N.c_u32_p),
                                _ptr(cols["border_mean"], N.c_double_p), _ptr(cols["border_sd"], N.c_double_p), res.cap)

    def native(bdp, bip, below=False, slack=0):
        """through the C entry points themselves, with exactly the bound as capacity"""
        if below:
            bound = int(L.dyn_format_csv_bound_samples(al._h, n, C.byref(res._c), None, None, bdp, None, rids, sids))
        else:
            bound = int(L.dyn_format_csv_bound_intervals(al._h, n, C.byref(res._c), None, None, bdp, None, bip, rids, sids))
        out = np.full(bound + 64, 0x5a, dtype=np.uint8)
        b0, e0 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        tail = ("".join(seqs).encode(), _ptr(seq_off, N.c_u64_p), rids, sids, so.ctypes.data_as(C.POINTER(C.c_int64)),
                li.ctypes.data_as(C.POINTER(C.c_int64)), 2, out.ctypes.data, bound - slack, _ptr(b0, N.c_u64_p), _ptr(e0, N.c_u64_p))
        if below:
            rc = L.dyn_format_csv_samples(al._h, n, C.byref(res._c), None, None, bdp, None, *tail)
        else:
            rc = L.dyn_format_csv_intervals(al._h, n, C.byref(res._c), None, None, bdp, None, bip, *tail)
        if slack:
            return rc
        assert rc == 0
        assert (out[bound:] == 0x5a).all() and int(e0.max()) <= bound                 # the bound bounds the output
        return b"".join(bytes(out[int(b0[i]):int(e0[i])]) for i in range(n))

    for bdp in (None, C.byref(bd)):
        below = native(bdp, None, below=True)
        assert native(bdp, None) == below                                            # bi == NULL: dyn_format_csv_samples' bytes
        want = _with_intervals(below.split(b"\n")[:-1], res, cols, starts)
        assert native(bdp, C.byref(bi)) == want                                      # after the other optional columns
    assert b",4294967295," in want or str(2 ** 32 - 1 + starts[0]).encode() in want
    assert native(None, C.byref(bi), slack=1) == N.DYN_ERR_INVALID_ARGUMENT          # too small a buffer: refused
    # the Python wrapper follows the result object's columns
    for on in (False, True):
        for c in COLS:
            setattr(res, c, cols[c] if on else None)
        buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
        plain = native(None, None, below=True)
        assert bytes(buf[:int(end[-1])]) == (_with_intervals(plain.split(b"\n")[:-1], res, cols, starts) if on else plain)
    # a column pointer missing: refused, nothing written
    broken = N.DynBorderIntervalOut(_ptr(cols["border_lo"], N.c_u32_p), None, _ptr(cols["border_mean"], N.c_double_p),
                                    _ptr(cols["border_sd"], N.c_double_p), res.cap)
    assert int(L.dyn_format_csv_bound_intervals(al._h, n, C.byref(res._c), None, None, None, None, C.byref(broken), rids, sids)) == 0
    al.close()


HEADER = b"readid,signalid,start,end,basepos,base,motif,state,posterior_probability,polish"
PARTS = {1: b",level_mean,level_stdv,level_median", 2: b",median_delta,mad_delta,homogeneity",
         8: b",border_probability,border_window_probability", 16: b",sample_starts",
         N.DYN_CSV_BORDER_INTERVAL: b",border_lo,border_hi,border_mean,border_sd"}


@pytest.mark.parametrize("extra", [0, 1, 3, 8, 0x1b])
def test_sink_header(tmp_path, extra):
    flags = N.DYN_CSV_BORDER_INTERVAL | extra
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    out = str(tmp_path / "o.csv.zst")
    assert L.dyn_csv_sink_open_ex(out.encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags, C.byref(h), err, 1024) == 0, err.value
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    text = zstd_io.decompress(open(out, "rb").read())
    assert text == HEADER + b"".join(PARTS[b] for b in sorted(PARTS) if flags & b) + b"\n"


@pytest.mark.parametrize("flags", [0x80, 0xc0, 0x44, 0x60, 0x140])
def test_sink_refuses_unassigned_flags(tmp_path, flags):
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags,
                                C.byref(h), err, 1024)
    assert rc == N.DYN_ERR_INVALID_ARGUMENT and b"unknown flags" in err.value and not h.value


def test_cli_flag_parses():
    from dynamont_amd.segmentation.segment import CSV_COLUMNS_INTERVALS, parse
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert parse(base).border_interval == 0
    assert parse(base + ["--border-interval", "0.9"]).border_interval == 0.9
    assert parse(base + ["--border-interval", "0.9", "--rescale-iters", "1", "--segment-scores", "4"]).border_interval == 0.9
    assert CSV_COLUMNS_INTERVALS == PARTS[N.DYN_CSV_BORDER_INTERVAL]
    for bad in (["--border-interval", "1.0"], ["--border-interval", "0.001"], ["--border-interval", "-0.5"],
                ["--border-interval", "0.9", "--border-confidence", "8"], ["--border-interval", "0.9", "--posterior-samples", "4"],
                ["--border-interval", "0.9", "--guide-auto", "16"], ["--border-interval", "0.9", "--guide-rescue", "16"]):
        with pytest.raises(SystemExit):
            parse(base + bad)


# ---- the yardstick itself --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(models):
    return bic.read_sets(models)


@pytest.fixture(scope="module")
def yards(models, sets, oracle_built):
    cache = {}
    return lambda name: bic.make_yards(models, sets, name, cache)


NAMES = ("plain", "plain_band50", "long", "long_band50", "imperfect", "imperfect_band50")


def test_read_sets_are_the_stated_ones(sets):
    assert set(sets) == set(NAMES)
    assert [len(sets[n][3]) for n in NAMES] == [6, 6, 3, 3, 4, 4]
    assert all(len(r.sequence) - 9 + 2 > 448 for r in sets["long"][3])               # more than 448 columns: the slots wrap


def test_every_column_sums_to_one(yards):
    for name in ("plain", "long_band50", "imperfect"):
        y = yards(name)[0]
        assert not np.isfinite(y.lpm[0]).any() and not np.isfinite(y.lpm[:, 0]).any()
        worst = max(abs(math.fsum(math.exp(x) for x in y.lpm[1:, n]) - 1.0) for n in range(1, y.N))
        print(f"{name}: column masses within {worst:.2e} of 1")
        assert worst <= 1e-9, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_intervals_are_ordered_nested_and_consistent_with_the_window_mass(yards, name):
    for y in yards(name):
        got = {m: y.at(m) for m in bic.MASSES}
        for m in bic.MASSES:
            lo, hi, mean, sd, cols = got[m]
            assert (lo <= hi).all() and (sd >= 0).all() and len(lo) == y.N - 1
            assert (lo <= y.res["signal_positions"].max()).all() and (hi <= y.T - 2).all()
            # the called border lies in its column, and the mean within the column's rows
            assert all(c.S > 0.5 for c in cols) and (mean >= 0).all() and (mean <= y.T - 2).all()
        assert (got[0.999][0] <= got[0.5][0]).all() and (got[0.5][1] <= got[0.999][1]).all()      # 0.999 nests 0.5
        assert (got[0.9][0] <= got[0.5][0]).all() and (got[0.5][1] <= got[0.9][1]).all()
        # mean and spread do not depend on the mass
        assert np.array_equal(got[0.5][2], got[0.999][2]) and np.array_equal(got[0.5][3], got[0.999][3])
        # the border confidence's window [r - W, r + W] that holds the whole interval holds its mass: C(hi) - C(lo - 1) >= mass
        for W in (2, 8, 64):
            wm = y.window_mass(W)
            for m in bic.MASSES:
                lo, hi = got[m][0].astype(np.int64) + 1, got[m][1].astype(np.int64) + 1          # rows
                inside = (y.rows - W <= lo) & (hi <= y.rows + W)
                assert (wm[inside] >= m - 1e-9).all(), (name, W, m)
                # ... and the other way round: a window that leaves less than `a` outside holds both quantiles
                full = wm >= 1.0 - (1.0 - m) / 2 + 1e-9
                assert inside[full].all(), (name, W, m)


def test_read_sets_have_the_properties_the_gpu_tests_state(yards):
    for group in (("plain",), ("long", "long_band50"), ("imperfect",), ("plain_band50",), ("imperfect_band50",)):
        ys = [y for name in group for y in yards(name)]
        bic.assert_conditions(ys, "+".join(group))
    for name in NAMES:
        for y in yards(name):
            assert abs(y.res["Z"]) < 1e6                                             # no far-out samples: the oracle's fp64 noise stays far below tol_C


def _effect(ys, wrong, mass=0.9):
    """(share of the borders whose lo or hi the wrong version changes, largest move of border_mean)"""
    changed = total = 0
    moved = 0.0
    for y in ys:
        lo, hi, mean, _, _ = y.at(mass)
        xlo, xhi, xmean, _, _ = y.at(mass, wrong)
        changed += int(((lo != xlo) | (hi != xhi)).sum())
        total += len(lo)
        moved = max(moved, float(np.abs(mean - xmean).max()))
    return changed / total, moved


@pytest.mark.parametrize("wrong", bic.MUTATIONS)
def test_wrong_versions_differ_from_the_yardstick(yards, wrong):
    """`>` for `>=`, a = 1 - mass, column n - 1, no band mask, row instead of row - 1: each changes at least 1 % of the borders or
    moves border_mean by more than 1e-3. Two of them need the ground they can bite on: without the band mask only a path along the
    band's edge gains mass (the imperfect reads at band 50: 2.3 % of the borders, 0 elsewhere), and `>` differs from `>=` only
    where a running sum MEETS its threshold, which none of about 12 000 does on the read sets -- so that one is held against
    bic.tie_lattice, where every column's sums meet both thresholds exactly."""
    if wrong == "greater_than":
        lpm, rows, last = bic.tie_lattice()
        lo, hi, mean, _, _ = bic.from_lpm(lpm, rows, last, 0.5)
        xlo, xhi, xmean, _, _ = bic.from_lpm(lpm, rows, last, 0.5, wrong)
        assert np.array_equal(lo, rows - 2) and np.array_equal(hi, rows)             # rows 1 and 3 of the four, as positions
        assert np.array_equal(xlo, lo + 1) and np.array_equal(xhi, hi + 1)           # `>`: every border changes
        for name in NAMES:                                                           # ... and recorded: nothing on the read sets
            share, moved = _effect(yards(name), wrong)
            assert share == 0.0 and moved == 0.0
        return
    names = ("imperfect_band50",) if wrong == "no_band_mask" else NAMES
    for name in names:
        share, moved = _effect(yards(name), wrong)
        print(f"{wrong} on {name}: {100 * share:.2f} % of the borders change, border_mean moves by up to {moved:.3g}")
        assert share >= 0.01 or moved > 1e-3, (wrong, name, share, moved)


def test_mutations_can_fail(yards):
    """the unmutated yardstick against itself differs by nothing: the comparison above is not vacuous"""
    y = yards("imperfect_band50")[0]
    a, b = y.at(0.9), bic.from_lpm(y.lpm, y.rows, y.last, 0.9, None)
    assert all(np.array_equal(a[k], b[k]) for k in range(4))
    assert _effect([y], None) == (0.0, 0.0)


def test_acceptance_rule_is_total_and_tight(yards):
    """the oracle's own rows are accepted; a row further off than the running sum allows is not"""
    for name in ("plain", "imperfect_band50"):
        for y in yards(name):
            lo, hi, _, _, cols = y.at(0.9)
            for j, c in enumerate(cols):
                last = int(y.last[j + 1])
                assert bic.accepts(c, 0.05, int(lo[j]) + 1, last) and bic.accepts(c, 0.95, int(hi[j]) + 1, last)
                if not c.near(0.05):
                    assert not bic.accepts(c, 0.05, int(lo[j]), last) and not bic.accepts(c, 0.05, int(lo[j]) + 2, last)
