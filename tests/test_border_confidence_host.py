"""CPU: the host half of the per-border posterior confidence (dyn_aligner_set_border_confidence). The new symbols resolve and
the switch is range-checked with a message; dyn_format_csv_borders writes Python's f"{x:.6f}" (0, 1 and a few ulps above 1
included), with bd == NULL the bytes of dyn_format_csv_scores, and its bound holds; the sink knows its new flag. The yardstick
of the GPU tests (tests/border_confidence_cases.py) is held against itself: every lattice column's masses sum to 1, the read
sets have the properties the GPU tests rely on, and four deliberately wrong versions each differ from it by more than 1e-3.
(The sink's refusal of a ticket submitted with the switch off needs a ticket, and a host-only handle creates none:
tests/test_gpu_border_confidence.py holds it.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import border_confidence_cases as bcc
from conftest import ROOT
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd import _native as N
from dynamont_amd._dynamont import AlignBatchResult, _ptr, format_csv
from dynamont_amd.segmentation.utils import segmentation_to_string

pytestmark = pytest.mark.usefixtures("native_lib")

COLS = ("border_probability", "border_window_probability")


def test_symbols_and_constants(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_border_confidence", "dyn_batch_fetch_borders", "dyn_format_csv_borders",
                 "dyn_format_csv_bound_borders"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "typedef struct dyn_border_out" in hdr and "DYN_BORDER_CONFIDENCE_MAX_WINDOW 256" in hdr
    assert "DYN_CSV_BORDER_CONFIDENCE 0x8u" in hdr and "DYN_ABI_VERSION 10" in hdr
    assert N.DYN_CSV_BORDER_CONFIDENCE == 8 and N.DYN_BORDER_CONFIDENCE_MAX_WINDOW == 256
    assert [f[0] for f in N.DynBorderOut._fields_] == ["border_probability", "border_window_probability", "capacity"]


def test_switch_range_and_null_on_a_host_handle(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    assert al._border_confidence == 0
    for bad in (-1, 257):
        with pytest.raises(ValueError, match=r"dyn_aligner_set_border_confidence: window must be 0 \.\. 256, got " + str(bad)):
            al.set_border_confidence(bad)
    assert al._border_confidence == 0
    for ok in (0, 1, 256, 0):
        al.set_border_confidence(ok)
        assert al._border_confidence == ok
    L = N.lib()
    assert L.dyn_aligner_set_border_confidence(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    col = np.zeros(4)
    assert L.dyn_batch_fetch_borders(None, C.byref(N.DynBorderOut(_ptr(col, N.c_double_p), _ptr(col, N.c_double_p), 4))) == \
        N.DYN_ERR_INVALID_ARGUMENT
    al.close()


# ---- the formatter ---------------------------------------------------------------------------------------------------------------
ABOVE_ONE = [np.nextafter(1.0, 2.0), 1.0 + 4 * 2.0 ** -52, 1.0000000000167653]
SPECIAL = [0.0, 1.0] + ABOVE_ONE + [5e-324, 0.0000005, 0.0000015, 0.9999995, 0.99999949, 0.5, 0.1234565] + [k / 128 for k in range(0, 129, 7)]


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
    cols = {"level_mean": -v[::-1].copy(), "level_stdv": np.roll(v, 5), "level_median": np.roll(v, 11),
            "median_delta": np.roll(v, 2), "mad_delta": np.roll(v, 3), "homogeneity": np.roll(v, 7),
            "border_probability": v.copy(), "border_window_probability": np.roll(v, 13)}
    cols["homogeneity"][::5] = np.nan
    return res, seqs, cols


def _python_rows(res, seqs, rid, sid, starts, last, k, rna, cols, levels, scores, borders):
    out = []
    for i in range(res.n):
        if res.status[i] != 0:
            continue
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        d = {"sequence_positions": res.sequence_positions[a:b], "signal_positions": res.signal_positions[a:b],
             "probabilities": res.probabilities[a:b], "states": ["M"] * (b - a)}
        lv = tuple(cols[c][a:b] for c in ("level_mean", "level_stdv", "level_median")) if levels else None
        lines = segmentation_to_string(d, rid[i], sid[i], starts[i], last[i], seqs[i], k, rna, levels=lv).split(b"\n")[:-1]
        assert len(lines) == b - a
        for j, line in enumerate(lines):
            if scores:
                line += ",{:.6f},{:.6f},{:.6f}".format(*(cols[c][a + j] for c in ("median_delta", "mad_delta", "homogeneity"))).encode()
            if borders:
                line += f",{cols['border_probability'][a + j]:.6f},{cols['border_window_probability'][a + j]:.6f}".encode()
            out.append(line + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna004", 9)])
def test_native_rows_equal_python_rows(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    rng = np.random.default_rng(5)
    values = SPECIAL + list(rng.random(200))
    n = 12
    res, seqs, cols = _fake_result(rng, n, values)
    rid = [f"r{i}" for i in range(n)]
    sid = [f"s{i}" for i in range(n)]
    starts = [int(x) for x in rng.integers(0, 100, n)]
    last = [starts[i] + int(res.signal_positions[int(res.seg_offsets[i]) + max(0, int(res.n_segments[i]) - 1)]) + 50 for i in range(n)]
    rna = pore.startswith("rna")
    L = N.lib()
    rids = (C.c_char_p * n)(*[x.encode() for x in rid])
    sids = (C.c_char_p * n)(*[x.encode() for x in sid])
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seqs])
    so, li = np.array(starts, dtype=np.int64), np.array(last, dtype=np.int64)
    ev = N.DynEventOut(*(_ptr(cols[c], N.c_double_p) for c in ("level_mean", "level_stdv", "level_median")), res.cap)
    sc = N.DynScoreOut(*(_ptr(cols[c], N.c_double_p) for c in ("median_delta", "mad_delta", "homogeneity")), res.cap)
    bd = N.DynBorderOut(*(_ptr(cols[c], N.c_double_p) for c in COLS), res.cap)

    def native(evp, scp, bdp, old=False, slack=0):
        """through the C entry points themselves, with exactly the bound as capacity; (bytes, bound, bytes written)"""
        if old:
            bound = int(L.dyn_format_csv_bound_scores(al._h, n, C.byref(res._c), evp, scp, rids, sids))
        else:
            bound = int(L.dyn_format_csv_bound_borders(al._h, n, C.byref(res._c), evp, scp, bdp, rids, sids))
        out = np.full(bound + 64, 0x5a, dtype=np.uint8)
        b0, e0 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        tail = ("".join(seqs).encode(), _ptr(seq_off, N.c_u64_p), rids, sids, so.ctypes.data_as(C.POINTER(C.c_int64)),
                li.ctypes.data_as(C.POINTER(C.c_int64)), 2, out.ctypes.data, bound - slack, _ptr(b0, N.c_u64_p), _ptr(e0, N.c_u64_p))
        if old:
            rc = L.dyn_format_csv_scores(al._h, n, C.byref(res._c), evp, scp, *tail)
        else:
            rc = L.dyn_format_csv_borders(al._h, n, C.byref(res._c), evp, scp, bdp, *tail)
        if slack:
            return rc
        assert rc == 0
        assert (out[bound:] == 0x5a).all() and int(e0.max()) <= bound                 # the bound bounds the output
        return b"".join(bytes(out[int(b0[i]):int(e0[i])]) for i in range(n))

    want = {(lv, s, b): _python_rows(res, seqs, rid, sid, starts, last, k, rna, cols, lv, s, b)
            for lv in (False, True) for s in (False, True) for b in (False, True)}
    assert b",1.000000,0.000000\n" in want[False, False, True] or b",0.000000," in want[False, False, True]
    for lv in (False, True):
        for s in (False, True):
            evp, scp = (C.byref(ev) if lv else None), (C.byref(sc) if s else None)
            assert native(evp, scp, C.byref(bd)) == want[lv, s, True]                   # after the level and score columns
            assert native(evp, scp, None) == want[lv, s, False]
            assert native(evp, scp, None) == native(evp, scp, None, old=True)           # bd == NULL: dyn_format_csv_scores' bytes
    # values a few ulps above 1 print as 1.000000, like Python's
    for x in ABOVE_ONE:
        assert f"{x:.6f}" == "1.000000"
    # too small a buffer: refused
    assert native(C.byref(ev), C.byref(sc), C.byref(bd), slack=1) == N.DYN_ERR_INVALID_ARGUMENT
    # the Python wrapper follows the result object's columns
    for b in (False, True):
        for c in COLS:
            setattr(res, c, cols[c] if b else None)
        buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
        assert bytes(buf[:int(end[-1])]) == want[False, False, b]
    # a column pointer missing: refused, nothing written
    broken = N.DynBorderOut(_ptr(cols["border_probability"], N.c_double_p), None, res.cap)
    assert int(L.dyn_format_csv_bound_borders(al._h, n, C.byref(res._c), None, None, C.byref(broken), rids, sids)) == 0
    al.close()


HEADER = b"readid,signalid,start,end,basepos,base,motif,state,posterior_probability,polish"
PARTS = {1: b",level_mean,level_stdv,level_median", 2: b",median_delta,mad_delta,homogeneity",
         8: b",border_probability,border_window_probability"}


@pytest.mark.parametrize("flags", [0, 1, 2, 3, 8, 9, 10, 11])
def test_sink_header(tmp_path, flags):
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    out = str(tmp_path / "o.csv.zst")
    assert L.dyn_csv_sink_open_ex(out.encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags, C.byref(h), err, 1024) == 0, err.value
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    text = zstd_io.decompress(open(out, "rb").read())
    assert text == HEADER + b"".join(PARTS[b] for b in (1, 2, 8) if flags & b) + b"\n"


def test_cli_flag_parses():
    from dynamont_amd.segmentation.segment import parse
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert parse(base).border_confidence == 0
    assert parse(base + ["--border-confidence", "8"]).border_confidence == 8
    with pytest.raises(SystemExit):
        parse(base + ["--border-confidence", "257"])


# ---- the yardstick itself --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracles(models, oracle_built):
    from oracle.pyoracle import Oracle
    cache = {}

    def get(pore, band=400):
        if (pore, band) not in cache:
            cache[pore, band] = Oracle(models["syn5"], synth.PORES[pore][0], band)
        return cache[pore, band]
    return get


def test_every_column_sums_to_one(models, oracles):
    r = bcc.plain_reads(models["syn5"], "rna002", bcc.RNA002_SEED, 1, 120)[0]
    lpm, res = bcc.lpm_columns(oracles("rna002"), r.signal, r.sequence)
    T, N = lpm.shape
    assert N == 117 and not np.isfinite(lpm[0]).any() and not np.isfinite(lpm[:, 0]).any()
    for n in range(1, N):
        total = math.fsum(math.exp(x) for x in lpm[1:, n])
        assert abs(total - 1.0) <= 1e-9, (n, total)
    # and the whole-read window is the column's sum
    rows = res["signal_positions"].astype(np.int64) + 1
    _, everything = bcc.from_lpm(lpm, rows, T)
    assert np.abs(everything - 1.0).max() <= 1e-9


def _sets(models):
    m = models["syn5"]
    return {
        "rna002": ("rna002", 400, 2, bcc.plain_reads(m, "rna002", bcc.RNA002_SEED, 3, 120)),
        "dna_r9": ("dna_r9", 400, 2, bcc.plain_reads(m, "dna_r9", bcc.DNA_R9_SEED, 3, 200)),
        "clipped": ("rna002", 400, 64, bcc.plain_reads(m, "rna002", bcc.CLIPPED_SEED, 3, 60)),
        "band50": ("dna_r9", 50, 256, bcc.imperfect_reads(m, "dna_r9", bcc.BAND50_SEED, 3, 200)),
        "band50_long": ("dna_r9", 50, 256, bcc.imperfect_reads(m, "dna_r9", bcc.BAND50_LONG_SEED, 1, 600)),
    }


def test_read_sets_have_the_properties_the_gpu_tests_state(models, oracles):
    sets = _sets(models)
    for name, (pore, band, W, reads) in sets.items():
        orc = oracles(pore, band)
        for r in reads:
            bp, bwp, res = bcc.yardstick(orc, r.signal, r.sequence, W, band)
            assert abs(res["Z"]) < 1e6                               # no far-out samples: the oracle's fp64 noise stays far below TOL
            T, N = len(r.signal) + 1, len(r.sequence) - orc.k + 2
            rows = res["signal_positions"].astype(np.int64) + 1
            clipped, leaving = bcc.window_counts(T, N, band, rows, W)
            assert (bp <= bwp + 1e-15).all() and bwp.max() <= 1.0 + 1e-9
            if name == "rna002":
                assert r.sequence.startswith("AAAAAAAAA")              # pad + A: a structural tie at the read's start
                assert bwp.min() <= 0.3 and bwp.max() >= 1.0 - bcc.TOL   # the values span 0.3 .. 1.0
            if name == "clipped":
                assert 12 <= clipped <= 13 and len(bp) == 56
            if name == "band50":
                assert 92 <= leaving <= 143 and len(bp) >= 196, leaving   # 92, 143 and 136 of 196 / 201 / 196 windows
                assert np.abs(bwp - 1.0).max() <= bcc.TOL                 # ... and every window still holds the whole column
            if name == "band50_long":
                assert N > 448 and leaving == 250 and 4 * leaving >= len(bp)   # 250 of 592; the band slots wrap


@pytest.mark.parametrize("wrong", bcc.MUTATIONS)
def test_wrong_versions_differ_from_the_yardstick(models, oracles, wrong):
    """window W - 1, window shifted by one row, column n - 1, no band mask: each moves at least one border of the read sets by
    more than 1e-3, a thousand tolerances"""
    worst = 0.0
    for name, (pore, band, W, reads) in _sets(models).items():
        if wrong == "no_band_mask" and band != 50:
            continue                                                   # (only those windows leave the band)
        orc = oracles(pore, band)
        for r in reads[:1]:
            bp, bwp, res = bcc.yardstick(orc, r.signal, r.sequence, W, band)
            xp, xwp, _ = bcc.yardstick(orc, r.signal, r.sequence, W, band, res=res, mutate=wrong)
            worst = max(worst, float(np.abs(xwp - bwp).max()), float(np.abs(xp - bp).max()))
    assert worst > 1e-3, (wrong, worst)


def test_mutations_can_fail(models, oracles):
    """the unmutated yardstick against itself differs by nothing: the comparison above is not vacuous"""
    pore, band, W, reads = _sets(models)["band50"]
    r = reads[0]
    a = bcc.yardstick(oracles(pore, band), r.signal, r.sequence, W, band)
    b = bcc.yardstick(oracles(pore, band), r.signal, r.sequence, W, band, res=a[2], mutate=None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
