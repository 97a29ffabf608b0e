"""CPU: the host half of the per-border segment scores (dyn_aligner_set_segment_scores). The NumPy restatement of the
definition (tests/segment_scores_cases.py) -- this feature's oracle -- equals the reference's scoring loop
(src/dynamont/misc/compareTools.py, processReadScores: np.median and scipy's median_abs_deviation over its windows) on the case
inputs after its float32 cast; L // 10 is its int(0.1 * L); five deliberately wrong readings of the definition each differ from
the right one on the case inputs; on a host-only handle the switch is range-checked with a message, the new formatter writes
Python's f"{x:.6f}" (nan included) with scores alone, levels alone and both, the old formatters write what they wrote, and the
sink knows its new flag. (The sink's refusal of a ticket submitted with the switch off needs a ticket, and a host-only handle
creates none: tests/test_gpu_segment_scores.py holds it.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import segment_scores_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd import _native as N
from dynamont_amd._dynamont import AlignBatchResult, _ptr, format_csv
from dynamont_amd.segmentation.utils import segmentation_to_string

pytestmark = pytest.mark.usefixtures("native_lib")


@pytest.fixture(scope="module")
def batch():
    return ssc.build_batch()


@pytest.fixture(scope="module")
def right(batch):
    """the restatement over the whole batch, once per window, shared and left unchanged"""
    return {W: ssc.reference(batch, W) for W in ssc.WINDOWS}


def test_symbols_and_constants(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_segment_scores", "dyn_batch_fetch_scores", "dyn_format_csv_scores", "dyn_format_csv_bound_scores"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "typedef struct dyn_score_out" in hdr and "DYN_SEGMENT_SCORES_MAX_WINDOW 256" in hdr and "DYN_CSV_SEGMENT_SCORES 0x2u" in hdr
    assert N.DYN_CSV_SEGMENT_SCORES == 2 and N.DYN_SEGMENT_SCORES_MAX_WINDOW == 256


# ---- against the reference --------------------------------------------------------------------------------------------------
def reference_scores(signal, borders, window):
    """what the reference's processReadScores computes for one read: for every border but the first and every segment but the
    last, the change of np.median and of scipy's MAD between the `window` samples before and after it, and the MAD of the
    segment with int(0.1 * length) samples (at least one) cut from either end, NaN below 10 samples; as float32"""
    mad = pytest.importorskip("scipy.stats").median_abs_deviation
    rows = []
    for i in range(1, len(borders) - 1):
        here, nxt = int(borders[i]), int(borders[i + 1])
        left = signal[max(0, here - window):here]
        right_ = signal[here:min(here + window, len(signal))]
        seg = signal[here:nxt]
        hom = np.nan
        if len(seg) >= 10:
            cut = max(int(0.1 * len(seg)), 1)
            hom = mad(seg[cut:-cut])
        rows.append((np.abs(np.median(right_) - np.median(left)), np.abs(mad(right_) - mad(left)), hom))
    return np.array(rows, dtype=np.float32).reshape(-1, 3)


def test_restatement_equals_the_reference_loop(batch, right):
    compared = 0
    for i, (name, x, sp, status) in enumerate(batch.reads):
        if status != 0 or len(sp) < 3:
            continue
        a = int(batch.read_seg_off[i])
        for W in ssc.WINDOWS if not name.startswith("small_") else (3, 64):
            ref = reference_scores(x, sp, W)
            ours = right[W][:, a + 1:a + len(sp) - 1].T.astype(np.float32)      # rows 1 .. n-2
            assert np.array_equal(ref.view(np.uint32) if ref.size else ref, ours.view(np.uint32) if ours.size else ours), (name, W)
            compared += len(ref)
    assert compared > 2000


def test_trim_is_the_references():
    L = np.arange(0, 5_000_001, dtype=np.int64)
    assert np.array_equal(L // 10, (0.1 * L).astype(np.int64))                   # int() truncates, as astype does for values >= 0


def test_restatement_on_small_cases():
    x = np.array([3.0, 1.0, 2.0, 10.0, 14.0, 12.0, 11.0])
    s = ssc.scores(x, [0, 3], 3)
    assert np.isnan(s[:, 0]).all() and ssc.bits(s[:, 0]).tolist() == [int(ssc.NAN_BITS)] * 3
    assert s[0, 1] == abs(12.0 - 2.0) and s[1, 1] == abs(2.0 - 1.0) and np.isnan(s[2, 1])   # B = 10, 14, 12 (cut by W)
    s = ssc.scores(x, [0, 3], 256)
    assert s[0, 1] == abs(11.5 - 2.0) and s[1, 1] == abs(1.0 - 1.0)                          # B = 10, 14, 12, 11: mad = (0.5 + 1.5) / 2
    y = np.arange(20.0) ** 2
    assert ssc.scores(y, [0], 5)[2, 0] == ssc.mad(y[2:18])
    assert ssc.scores(np.array([-0.0] * 12), [0, 1], 4)[:, 1].tolist() == [0.0, 0.0, 0.0]
    assert not np.signbit(ssc.scores(np.array([-0.0] * 12), [0, 1], 4)[:, 1]).any()


# ---- can the case inputs fail? ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong,columns", [("lower_median", (0, 1, 2)), ("left_inclusive", (0, 1)), ("trim_plus_one", (2,)),
                                           ("mad_about_mean", (1, 2)), ("windows_not_cut", (0, 1))])
def test_wrong_readings_differ_on_the_case_inputs(batch, right, wrong, columns):
    """(W = 3, not 2: the mean of two values is their median, so no window of two samples can tell those two apart)"""
    assert wrong in ssc.WRONG
    total = dict.fromkeys(columns, 0)
    for W in (3, 64, 256):
        bad = ssc.reference(batch, W, wrong)
        for c in columns:
            differ = ssc.bits(bad[c]) != ssc.bits(right[W][c])
            assert differ.any(), (wrong, W, c)
            total[c] += int(differ.sum())
        for c in set(range(3)) - set(columns):
            assert np.array_equal(ssc.bits(bad[c]), ssc.bits(right[W][c]))
    assert min(total.values()) >= 10, total


def test_case_inputs_hold_what_the_issue_names(batch, right):
    lens = np.concatenate([np.diff(np.append(sp, len(x))) for _, x, sp, st in batch.reads if st == 0])
    trimmed = lens - 2 * np.maximum(lens // 10, 1)
    for L in list(range(1, 12)) + [19, 20, 29, 30, 318, 319, 320, 321, 20000, 20001]:
        assert (lens == L).any(), L
    assert {ssc.SHORT_MAX, ssc.SHORT_MAX + 1} <= set(trimmed[lens >= 10].tolist())
    assert len(batch.read) == 300 and (batch.status != 0).sum() >= 2 and sorted(batch.read.tolist()) == list(range(300))
    assert any(len(sp) == 1 for _, _, sp, _ in batch.reads) and any(len(x) < 63 for _, x, _, _ in batch.reads)
    r = right[64]
    assert (r[2] == 0.0).sum() >= 5 and (r[1] == 0.0).sum() >= 5                 # constant stretches: MAD 0
    assert np.signbit(batch.sig[batch.sig == 0.0]).any() and (np.abs(batch.sig[batch.sig != 0]) < 2.3e-308).any()
    assert not np.signbit(r[~np.isnan(r)]).any()                                   # never -0.0
    nan = np.isnan(r)
    assert np.array_equal(ssc.bits(r)[nan], np.full(int(nan.sum()), ssc.NAN_BITS))


def test_sliced_batch_and_its_reference():
    """The 65 541-descriptor batch of tests/test_gpu_segment_scores.py: its shape; its vectorised reference equals scores() read by
    read on a sample; and a second launch of k_score_window that is handed the first descriptors again (descs in place of
    descs + r0) shows in median_delta and mad_delta of every row of descriptors 65 535 .. 65 540."""
    b = ssc.build_sliced_batch()
    s = b.sliced
    n = len(b.read)
    assert n == ssc.SLICE + ssc.TAIL and sorted(b.read.tolist()) == list(range(n))
    bulk = np.ones(n, dtype=bool)
    bulk[s["long_reads"]] = False
    assert set((s["S"][bulk] + 1).tolist()) == {3, 4, 5, 6} and set((s["nseg"][bulk] + 1).tolist()) == {2, 3}
    assert np.array_equal(np.sort(b.read[ssc.SLICE:]), s["tail"]) and np.isin(s["long_reads"], b.read[:ssc.SLICE]).sum() == 3
    assert (b.status[s["long_reads"]] == 0).all() and (b.status != 0).sum() == 300
    rng = np.random.default_rng(9)
    sample = np.concatenate([rng.choice(np.flatnonzero(bulk), 400, replace=False), s["long_reads"]])
    tail_rows = np.concatenate([np.arange(int(b.read_seg_off[i]), int(b.read_seg_off[i]) + 3) for i in s["tail"]])
    for W in ssc.SLICED_WINDOWS:
        want = ssc.reference_sliced(b, W)
        for i in sample:
            a, m = int(b.read_seg_off[i]), int(s["nseg"][i])
            x = b.sig[int(b.read_sig_off[i]):int(b.read_sig_off[i]) + int(s["S"][i])]
            one = ssc.scores(x, b.segrow[a:a + m].astype(np.int64) - 1, W) if b.status[i] == 0 else np.zeros((3, m))
            assert np.array_equal(ssc.bits(want[:, a:a + m]), ssc.bits(one)), (W, i)
        assert np.isfinite(want[:2, tail_rows[1::3]]).all() and np.isfinite(want[2, tail_rows]).all()
        other = ssc.reference_sliced(b, W, skip_descs=np.arange(ssc.SLICE, n))
        assert (ssc.bits(other[:2, tail_rows]) != ssc.bits(want[:2, tail_rows])).all()
        assert np.array_equal(ssc.bits(other[2]), ssc.bits(want[2]))               # homogeneity: no sliced launch
    assert not np.array_equal(ssc.bits(ssc.reference_sliced(b, 8)), ssc.bits(ssc.reference_sliced(b, 64)))


@pytest.mark.parametrize("pore", ["dna_r9", "rna004"])
def test_random_read_seeds_meet_the_gpu_tests_condition(models, oracle_built, pore):
    """tests/test_gpu_segment_scores.py asserts that at least 25 % of the rows of its random reads have a finite homogeneity and
    that every delta row but each read's first is finite: true of the CPU oracle's borders for those seeds (with Poisson(10)
    dwells P(L >= 10) is about 0.54), so a GPU run that misses it has lost rows, not luck."""
    from conftest import model_for
    from oracle.pyoracle import Oracle
    seed, n = ssc.RANDOM_READS[pore]
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(seed, n, pore, mean, sd, (60, 400))
    orc = Oracle(model, synth.PORES[pore][0])
    rows = finite_h = 0
    for r in reads:
        sp = orc.align(r.signal, r.sequence, True)["signal_positions"]
        s = ssc.scores(r.signal, sp, 8)
        assert np.isnan(s[:2, 0]).all() and np.isfinite(s[:2, 1:]).all()
        rows += len(sp)
        finite_h += int(np.isfinite(s[2]).sum())
    assert rows > 16 * 50 and finite_h >= 0.35 * rows, (rows, finite_h)      # with room above the GPU tests' 25 %


# ---- the host-only handle -----------------------------------------------------------------------------------------------------
def test_switch_range_on_a_host_handle(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    assert al._segment_scores == 0
    for bad in (-1, 257):
        with pytest.raises(ValueError, match="window must be 0 .. 256"):
            al.set_segment_scores(bad)
    assert al._segment_scores == 0
    for ok in (0, 1, 256, 0):
        al.set_segment_scores(ok)
        assert al._segment_scores == ok
    assert N.lib().dyn_aligner_set_segment_scores(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    al.close()


SPECIAL = [np.nan, 0.0, 5e-324, 1e20, 1e300, 1.7976931348623157e308, 511.9999995, 512.0000005, 0.0000005, 0.0000015, 1e15,
           1e15 - 0.5, 999999999999999.9] + [k / 128 for k in range(0, 300, 7)]


def _fake_result(rng, n_reads, values):
    """an AlignBatchResult with rows as the GPU fills them; level and score columns holding `values` (cycled, shifted)"""
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
            "median_delta": v.copy(), "mad_delta": np.roll(v, 3), "homogeneity": np.roll(v, 7)}
    for c in ("level_mean", "level_stdv", "level_median"):
        cols[c][np.isnan(cols[c])] = 0.25   # the level columns are finite
    return res, seqs, cols


def _python_rows(res, seqs, rid, sid, starts, last, k, rna, cols, levels, scores):
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
            out.append(line + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna004", 9)])
def test_native_rows_equal_python_rows(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    rng = np.random.default_rng(5)
    values = SPECIAL + list(np.abs(rng.normal(0, 1, 200))) + list(np.abs(rng.normal(0, 1, 50)) * 1e6)
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

    def native(evp, scp, old=None):
        """through the C entry points themselves, with exactly the bound as capacity"""
        if old == "events":
            bound = int(L.dyn_format_csv_bound_events(al._h, n, C.byref(res._c), evp, rids, sids))
        elif old == "plain":
            bound = int(L.dyn_format_csv_bound(al._h, n, C.byref(res._c), rids, sids))
        else:
            bound = int(L.dyn_format_csv_bound_scores(al._h, n, C.byref(res._c), evp, scp, rids, sids))
        out = np.zeros(bound, dtype=np.uint8)
        b0, e0 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        tail = ("".join(seqs).encode(), _ptr(seq_off, N.c_u64_p), rids, sids, so.ctypes.data_as(C.POINTER(C.c_int64)),
                li.ctypes.data_as(C.POINTER(C.c_int64)), 2, out.ctypes.data, bound, _ptr(b0, N.c_u64_p), _ptr(e0, N.c_u64_p))
        if old == "events":
            rc = L.dyn_format_csv_events(al._h, n, C.byref(res._c), evp, *tail)
        elif old == "plain":
            rc = L.dyn_format_csv(al._h, n, C.byref(res._c), *tail)
        else:
            rc = L.dyn_format_csv_scores(al._h, n, C.byref(res._c), evp, scp, *tail)
        assert rc == 0
        return b"".join(bytes(out[int(b0[i]):int(e0[i])]) for i in range(n))

    want = {(lv, s): _python_rows(res, seqs, rid, sid, starts, last, k, rna, cols, lv, s) for lv in (False, True) for s in (False, True)}
    assert b",nan" in want[False, True] and b"nan" not in want[True, False]
    assert native(None, C.byref(sc)) == want[False, True]                        # scores alone
    assert native(C.byref(ev), None) == want[True, False]                        # levels alone
    assert native(C.byref(ev), C.byref(sc)) == want[True, True]                  # both: the scores after the levels
    assert native(None, None) == want[False, False]
    assert native(C.byref(ev), None, old="events") == want[True, False]          # the old entry points: what they wrote
    assert native(None, None, old="events") == want[False, False]
    assert native(None, None, old="plain") == want[False, False]
    # the Python wrapper follows the result object's columns
    for lv in (False, True):
        for s in (False, True):
            for c in ("level_mean", "level_stdv", "level_median"):
                setattr(res, c, cols[c] if lv else None)
            for c in ("median_delta", "mad_delta", "homogeneity"):
                setattr(res, c, cols[c] if s else None)
            buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
            assert bytes(buf[:int(end[-1])]) == want[lv, s]
    # a column pointer missing: refused, nothing written
    broken = N.DynScoreOut(_ptr(cols["median_delta"], N.c_double_p), None, _ptr(cols["homogeneity"], N.c_double_p), res.cap)
    assert int(L.dyn_format_csv_bound_scores(al._h, n, C.byref(res._c), None, C.byref(broken), rids, sids)) == 0
    al.close()


@pytest.mark.parametrize("flags,columns", [(0, b""), (1, b",level_mean,level_stdv,level_median"),
                                           (2, b",median_delta,mad_delta,homogeneity"),
                                           (3, b",level_mean,level_stdv,level_median,median_delta,mad_delta,homogeneity")])
def test_sink_header(tmp_path, flags, columns):
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    out = str(tmp_path / "o.csv.zst")
    assert L.dyn_csv_sink_open_ex(out.encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags, C.byref(h), err, 1024) == 0, err.value
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    text = zstd_io.decompress(open(out, "rb").read())
    assert text == b"readid,signalid,start,end,basepos,base,motif,state,posterior_probability,polish" + columns + b"\n"


def test_sink_refuses_an_unknown_flag(tmp_path):
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = N.lib().dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, 4,
                                      C.byref(h), err, 1024)
    assert rc == N.DYN_ERR_INVALID_ARGUMENT and b"unknown flags" in err.value
