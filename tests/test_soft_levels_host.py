"""CPU: the host half of the posterior-weighted per-base levels (dyn_aligner_set_soft_levels). The new symbols resolve;
dyn_format_csv_soft writes the three derived fields as Python's f"{x:.6f}" (a NaN as "nan"), with sl == NULL the bytes of
dyn_format_csv_intervals, and its bound holds; the sink knows its new flag and refuses the unassigned ones; every new refusal has
its text, on a handle without a device. The yardstick of the GPU tests (tests/soft_level_cases.py) is held against the
definition's invariants on all 26 reads of the six read sets -- every row's posterior sums to 1, the weights sum to T - 1, and
pooled per k-mer the three sums are Oracle.train's (and, where the compiled reference is there, the reference's own M-step) --
and six deliberately wrong versions each differ from it.
(The sink's refusal of a ticket submitted with the switch off needs a ticket, and a host-only handle creates none:
tests/test_gpu_soft_levels.py holds it.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soft_level_cases as slc
from conftest import ROOT
from dynamont_amd import Aligner, guide as G, synth, zstd_io
from dynamont_amd import _native as N
from dynamont_amd._dynamont import AlignBatchResult, JobWants, _OPTIONAL, _ptr, format_csv, soft_level_columns

pytestmark = pytest.mark.usefixtures("native_lib")

COLS = ("soft_weight", "soft_sum", "soft_sumsq")
NEW = ("dyn_aligner_set_soft_levels", "dyn_batch_fetch_soft_levels", "dyn_format_csv_soft", "dyn_format_csv_bound_soft")


def test_symbols_and_constants(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "DYN_ABI_VERSION 10" in hdr
    m = re.search(r"typedef struct dyn_soft_level_out \{(.*?)\} dyn_soft_level_out;", hdr, re.S)
    assert m and re.findall(r"(double\*|uint64_t) (\w+);", m.group(1)) == \
        [("double*", "weight"), ("double*", "sum"), ("double*", "sumsq"), ("uint64_t", "capacity")]
    assert "DYN_CSV_SOFT_LEVELS 0x200u" in hdr and N.DYN_CSV_SOFT_LEVELS == 0x200
    assert [f[0] for f in N.DynSoftLevelOut._fields_] == ["weight", "sum", "sumsq", "capacity"]
    assert "soft" in JobWants._fields and [c[0] for c in _OPTIONAL["soft"][0]] == list(COLS)
    for key in COLS:
        assert getattr(AlignBatchResult(1, 1), key) is None                          # off: no columns


def test_null_arguments_on_a_host_handle(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    assert al._soft_levels is False
    al.set_soft_levels(True)
    assert al._soft_levels is True and al._job_wants(True).soft is True and not al._job_wants(False).soft
    al.set_soft_levels(False)
    assert not al._job_wants(True).soft
    L = N.lib()
    assert L.dyn_aligner_set_soft_levels(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    d = np.zeros(4)
    out = N.DynSoftLevelOut(_ptr(d, N.c_double_p), _ptr(d, N.c_double_p), _ptr(d, N.c_double_p), 4)
    assert L.dyn_batch_fetch_soft_levels(None, C.byref(out)) == N.DYN_ERR_INVALID_ARGUMENT
    al.close()
    nt = Aligner(models["syn9"], "rna004", mode="resquiggle", device="host")         # modes ntk / resquiggle ignore the switch
    nt.set_soft_levels(True)
    assert not nt._job_wants(True).soft
    nt.close()


# ---- the refusals: every new one, on a handle without a device --------------------------------------------------------------------
SOFT = "dyn_aligner_set_soft_levels"
OTHERS = {
    "confidence": (lambda al: al.set_border_confidence(8), lambda al: al.set_border_confidence(0), "dyn_aligner_set_border_confidence(a, window > 0)"),
    "samples": (lambda al: al.set_posterior_samples(4, 11), lambda al: al.set_posterior_samples(0), "dyn_aligner_set_posterior_samples(a, count > 0)"),
    "auto_guide": (lambda al: al.set_auto_guide(16), lambda al: al.set_auto_guide(0), "dyn_aligner_set_auto_guide(a, half_width > 0)"),
    "rescue": (lambda al: al.set_guide_rescue(1, 16), lambda al: al.set_guide_rescue(0, 0), "dyn_aligner_set_guide_rescue(a, half_width > 0)"),
    "interval": (lambda al: al.set_border_interval(0.9), lambda al: al.set_border_interval(0), "dyn_aligner_set_border_interval(a, mass > 0)"),
}
COMBINES = {
    "rescale": (lambda al: al.set_rescale(2), lambda al: al.set_rescale(0)),
    "event_stats": (lambda al: al.set_event_stats(True), lambda al: al.set_event_stats(False)),
    "scores": (lambda al: al.set_segment_scores(8), lambda al: al.set_segment_scores(0)),
}
NO_GPU = "no GPU bound to this handle"                                              # (the k-mer summary's and the band margins' setters need a device: GPU test)


def outcome(call):
    with pytest.raises((ValueError, RuntimeError)) as e:
        call()
    return type(e.value), str(e.value)


def test_refusals_and_combinations_without_a_device(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    reads = synth.make_reads(4401, 3, "dna_r9", mean, sd, (20, 40))
    pk = synth.pack_reads(reads)
    al = Aligner(models["syn5"], "dna_r9", device="host")
    al.set_soft_levels(True)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        runs = (("dyn_batch_align", b.align), ("dyn_batch_align_async", lambda calc: al.align_async(*pk, calc)))
        for name, (on, off, text) in OTHERS.items():
            on(al)
            try:
                for api, run in runs:
                    want = f"{api}: {SOFT} is on, which does not combine with {text}"
                    assert outcome(lambda: run(True)) == (ValueError, want), (api, name)
                    kind, msg = outcome(lambda: run(False))                          # the Z-only job reads none of the switches
                    assert kind is RuntimeError and NO_GPU in msg, (api, name, msg)
            finally:
                off(al)
        for name, (on, off) in COMBINES.items():
            on(al)
            try:
                for api, run in runs:
                    kind, msg = outcome(lambda: run(True))
                    assert kind is RuntimeError and NO_GPU in msg, (api, name, msg)
            finally:
                off(al)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:      # a guided batch
        b.set_guide(np.concatenate([G.diagonal_guide(len(r.signal), len(r.sequence) - 5 + 2) for r in reads]), 8)
        assert outcome(lambda: b.align(True)) == (ValueError, "dyn_batch_align: the batch carries a guide (dyn_batch_set_guide / "
                                                  "dyn_batch_auto_guide), which does not combine with dyn_aligner_set_soft_levels(a, 1)")
    al.set_soft_levels(False)
    al.close()


# ---- the formatter ---------------------------------------------------------------------------------------------------------------
def _fake_result(rng, n_reads):
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
    w = rng.random(cap) * 40.0 + 0.5
    mean = rng.normal(0.0, 1.5, cap)
    var = rng.random(cap) * 0.3
    cols = {"soft_weight": w, "soft_sum": w * mean, "soft_sumsq": w * (var + mean * mean),
            "border_lo": rng.integers(0, 1000, cap).astype(np.uint32), "border_hi": rng.integers(0, 1000, cap).astype(np.uint32),
            "border_mean": rng.random(cap) * 100, "border_sd": rng.random(cap)}
    # the edges: weight 0 (NaN mean and stdv), a variance below the clamp, a negative one by rounding, a large weight
    cols["soft_weight"][:4] = (0.0, 2.0, 3.0, 1e15)
    cols["soft_sum"][:4] = (0.0, 1.0, 3.0, 1e15)
    cols["soft_sumsq"][:4] = (0.0, 0.5, 2.9999999999, 1e15)
    return res, seqs, cols


def _with_soft(lines, res, cols):
    """the rows of the formatter below with ',{soft_dwell:.6f},{soft_mean:.6f},{soft_stdv:.6f}' appended"""
    out, k = [], 0
    for i in range(res.n):
        if res.status[i] != 0:
            continue
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        dwell, mean, stdv = soft_level_columns(cols["soft_weight"][a:a + m], cols["soft_sum"][a:a + m], cols["soft_sumsq"][a:a + m])
        for j in range(m):
            out.append(lines[k] + f",{dwell[j]:.6f},{mean[j]:.6f},{stdv[j]:.6f}".encode())
            k += 1
    assert k == len(lines)
    return b"".join(x + b"\n" for x in out)


@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna004", 9)])
def test_native_rows_and_bound(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    rng = np.random.default_rng(5)
    n = 12
    res, seqs, cols = _fake_result(rng, n)
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
    bi = N.DynBorderIntervalOut(_ptr(cols["border_lo"], N.c_u32_p), _ptr(cols["border_hi"], N.c_u32_p),
                                _ptr(cols["border_mean"], N.c_double_p), _ptr(cols["border_sd"], N.c_double_p), res.cap)
    sl = N.DynSoftLevelOut(*[_ptr(cols[c], N.c_double_p) for c in COLS], res.cap)

    def native(bip, slp, below=False, slack=0):
        """through the C entry points themselves, with exactly the bound as capacity"""
        if below:
            bound = int(L.dyn_format_csv_bound_intervals(al._h, n, C.byref(res._c), None, None, None, None, bip, rids, sids))
        else:
            bound = int(L.dyn_format_csv_bound_soft(al._h, n, C.byref(res._c), None, None, None, None, bip, slp, rids, sids))
        out = np.full(bound + 64, 0x5a, dtype=np.uint8)
        b0, e0 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        tail = ("".join(seqs).encode(), _ptr(seq_off, N.c_u64_p), rids, sids, so.ctypes.data_as(C.POINTER(C.c_int64)),
                li.ctypes.data_as(C.POINTER(C.c_int64)), 2, out.ctypes.data, bound - slack, _ptr(b0, N.c_u64_p), _ptr(e0, N.c_u64_p))
        if below:
            rc = L.dyn_format_csv_intervals(al._h, n, C.byref(res._c), None, None, None, None, bip, *tail)
        else:
            rc = L.dyn_format_csv_soft(al._h, n, C.byref(res._c), None, None, None, None, bip, slp, *tail)
        if slack:
            return rc
        assert rc == 0
        assert (out[bound:] == 0x5a).all() and int(e0.max()) <= bound                 # the bound bounds the output
        return b"".join(bytes(out[int(b0[i]):int(e0[i])]) for i in range(n))

    for bip in (None, C.byref(bi)):
        below = native(bip, None, below=True)
        assert native(bip, None) == below                                            # sl == NULL: dyn_format_csv_intervals' bytes
        want = _with_soft(below.split(b"\n")[:-1], res, cols)
        assert native(bip, C.byref(sl)) == want                                      # after every other optional column
    assert b",0.000000,nan,nan\n" in want and b",2.000000,0.500000,0.000001\n" in want    # weight 0; the 1e-12 clamp
    assert b",3.000000,1.000000,0.000001\n" in want and b"-nan" not in want               # a variance below 0 by rounding
    assert native(None, C.byref(sl), slack=1) == N.DYN_ERR_INVALID_ARGUMENT          # too small a buffer: refused
    # the Python wrapper follows the result object's columns
    for on in (False, True):
        for c in COLS:
            setattr(res, c, cols[c] if on else None)
        buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
        plain = native(None, None, below=True)
        assert bytes(buf[:int(end[-1])]) == (_with_soft(plain.split(b"\n")[:-1], res, cols) if on else plain)
    # read(i) derives the same three values
    d = res.read(0)
    a, m = int(res.seg_offsets[0]), int(res.n_segments[0])
    want3 = soft_level_columns(*[cols[c][a:a + m] for c in COLS])
    for key, w in zip(("soft_dwell", "soft_mean", "soft_stdv"), want3):
        assert np.array_equal(d[key], w, equal_nan=True), key
    assert np.isnan(d["soft_mean"][0]) and np.isnan(d["soft_stdv"][0]) and d["soft_dwell"][0] == 0.0
    # a column pointer missing: refused, nothing written
    broken = N.DynSoftLevelOut(_ptr(cols["soft_weight"], N.c_double_p), None, _ptr(cols["soft_sumsq"], N.c_double_p), res.cap)
    assert int(L.dyn_format_csv_bound_soft(al._h, n, C.byref(res._c), None, None, None, None, None, C.byref(broken), rids, sids)) == 0
    al.close()


HEADER = b"readid,signalid,start,end,basepos,base,motif,state,posterior_probability,polish"
PARTS = {1: b",level_mean,level_stdv,level_median", 2: b",median_delta,mad_delta,homogeneity",
         8: b",border_probability,border_window_probability", 16: b",sample_starts",
         0x40: b",border_lo,border_hi,border_mean,border_sd", N.DYN_CSV_SOFT_LEVELS: b",soft_dwell,soft_mean,soft_stdv"}


@pytest.mark.parametrize("extra", [0, 1, 3, 0x40, 0x5b])
def test_sink_header(tmp_path, extra):
    flags = N.DYN_CSV_SOFT_LEVELS | extra
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    out = str(tmp_path / "o.csv.zst")
    assert L.dyn_csv_sink_open_ex(out.encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags, C.byref(h), err, 1024) == 0, err.value
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    text = zstd_io.decompress(open(out, "rb").read())
    assert text == HEADER + b"".join(PARTS[b] for b in sorted(PARTS) if flags & b) + b"\n"


@pytest.mark.parametrize("flags", [0x4, 0x20, 0x80, 0x100, 0x400, 0x204, 0x220, 0x280, 0x300, 0x600])
def test_sink_refuses_unassigned_flags(tmp_path, flags):
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags,
                                C.byref(h), err, 1024)
    assert rc == N.DYN_ERR_INVALID_ARGUMENT and b"unknown flags" in err.value and not h.value


def test_cli_flag_parses():
    from dynamont_amd.segmentation.segment import CSV_COLUMNS_SOFT, parse
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert parse(base).soft_levels is False
    assert parse(base + ["--soft-levels"]).soft_levels is True
    assert parse(base + ["--soft-levels", "--rescale-iters", "1", "--segment-scores", "4", "--event-stats"]).soft_levels is True
    assert parse(base + ["--soft-levels", "--border-interval", "0.9"]).soft_levels is True      # refused by the library, not here
    assert CSV_COLUMNS_SOFT == PARTS[N.DYN_CSV_SOFT_LEVELS]


# ---- the yardstick itself --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(models):
    return slc.read_sets(models)


@pytest.fixture(scope="module")
def yards(models, sets, oracle_built):
    cache = {}
    return lambda name: slc.make_yards(models, sets, name, cache)


def test_read_sets_are_the_stated_ones(sets):
    assert set(sets) == set(slc.NAMES)
    assert [len(sets[n][3]) for n in slc.NAMES] == [6, 6, 3, 3, 4, 4]
    assert all(len(r.sequence) - 9 + 2 > 448 for r in sets["long"][3])               # more than 448 columns: the slots wrap


@pytest.mark.parametrize("name", slc.NAMES)
def test_invariants_of_the_definition(yards, name):
    """column 0 holds no mass in rows >= 1; every row's g sums to 1 within 6e-10; the weights sum to T - 1 within 1e-5; pooled per
    k-mer the three sums are Oracle.train's within 1e-12 relative; float32 log-posteriors stay inside the bounds; no weight is 0"""
    ys = yards(name)
    orc = ys[0].orc
    worst_row = worst_sum = worst_pool = worst_f32 = 0.0
    for y in ys:
        assert not np.isfinite(y.lpm[1:, 0]).any() and not np.isfinite(y.lpe[1:, 0]).any()
        assert not np.isfinite(y.lpm[0]).any()
        with np.errstate(invalid="ignore"):
            g = np.exp(y.lpm[1:]) + np.exp(y.lpe[1:])
        worst_row = max(worst_row, float(np.abs(np.cumsum(g, axis=1)[:, -1] - 1.0).max()))
        w, s1, s2, tw, t1, t2 = y.at()
        assert w.min() > 0 and len(w) == y.N - 1
        worst_sum = max(worst_sum, abs(float(np.cumsum(w)[-1]) - (y.T - 1)))
        tr = orc.train(y.signal, y.seq, dense=False)
        for mine, key in zip(y.pooled((w, s1, s2), orc.num_kmers), ("weight", "sum", "sumsq")):
            assert np.array_equal(mine == 0, tr[key] == 0), (name, key)               # the k-mers the read holds, no other
            live = tr[key] != 0
            worst_pool = max(worst_pool, float(np.max(np.abs(mine[live] - tr[key][live]) / np.abs(tr[key][live]))))
        fw, f1, f2, _, _, _ = y.at(fp32=True)
        worst_f32 = max(worst_f32, *(float(np.max(np.abs(a - b) / t)) for a, b, t in ((fw, w, tw), (f1, s1, t1), (f2, s2, t2))))
    print(f"{name}: rows within {worst_row:.1e} of 1, sum of weights within {worst_sum:.1e} of T - 1, pooled sums within "
          f"{worst_pool:.1e} relative of Oracle.train, float32 log-posteriors move a sum by {worst_f32:.2f} of its bound")
    assert worst_row <= 6e-10 and worst_sum <= 1e-5 and worst_pool <= 1e-12 and worst_f32 <= 1.0, (name, worst_row, worst_sum, worst_pool, worst_f32)


@pytest.mark.parametrize("name", ("plain", "long_band50", "imperfect", "imperfect_band50"))
def test_pooled_sums_give_the_references_m_step(models, sets, yards, name):
    """Where the compiled reference is there: its train() returns the M-step's mean and stdev per k-mer, which test_oracle_golden
    holds EQUAL to the oracle's (no tolerance). So the yardstick's pooled sums, which are the oracle's within 1e-12 relative, give
    the reference's mean within 1e-12 of the level scale and its variance within the bound that follows for s2 / w - m^2."""
    from oracle.pyoracle import Reference, reference_available
    if not reference_available():
        pytest.skip("the compiled reference (oracle/_ref) is not on this machine")
    key, pore, band, _ = sets[name]
    ref = Reference(models[key], synth.PORES[pore][0], band)
    for y in yards(name)[:2]:
        orc = y.orc
        rt, ot = ref.train(y.signal, y.seq, orc.num_kmers), orc.train(y.signal, y.seq)
        assert np.array_equal(rt["mean"], ot["mean"]) and np.array_equal(rt["stdev"], ot["stdev"])   # what the golden test grants: nothing
        pw, p1, p2 = y.pooled(y.at()[:3], orc.num_kmers)
        live = pw > 0
        mean = p1[live] / pw[live]
        var = p2[live] / pw[live] - mean * mean
        sd = np.sqrt(np.where(var < 1e-12, 1e-12, var))
        rel = 1e-12
        scale = np.abs(ot["sum"][live]) / pw[live] + np.abs(mean)                    # |d mean| <= rel * (|s1| / w + |mean|)
        assert (np.abs(mean - rt["mean"][live]) <= rel * scale + 1e-15).all()
        dvar = rel * 2 * (p2[live] / pw[live]) + 2 * np.abs(mean) * rel * scale
        assert (np.abs(sd ** 2 - rt["stdev"][live] ** 2) <= dvar + 1e-15).all()


@pytest.mark.parametrize("name", slc.NAMES)
def test_read_sets_show_what_the_feature_is_for(yards, name):
    """|soft_dwell - called dwell| > 0.5 samples on at least 10 % of the bases of every read set"""
    far = total = 0
    largest = 0.0
    for y in yards(name):
        d = np.abs(y.at()[0] - y.called_dwell())
        far, total, largest = far + int((d > 0.5).sum()), total + len(d), max(largest, float(d.max()))
    print(f"{name}: {100 * far / total:.1f} % of the bases differ by more than 0.5 samples, the largest difference {largest:.1f}")
    assert far >= 0.10 * total, (name, far, total)


def _moved(y, wrong):
    """share of the columns a wrong version moves out of a bound (what a device with that mistake would fail on)"""
    w, s1, s2, tw, t1, t2 = y.at()
    xw, x1, x2 = y.at(wrong)[:3]
    return float(np.mean((np.abs(xw - w) > tw) | (np.abs(x1 - s1) > t1) | (np.abs(x2 - s2) > t2)))


@pytest.mark.parametrize("wrong", slc.MUTATIONS)
def test_wrong_versions_differ_from_the_yardstick(yards, wrong):
    """pM alone, pE alone, x[t] for x[t-1], column n - 1: each must move at least half of the columns of every read set out of a
    bound (measured, the first two reads of every set: 100 % each, on all six sets). Without the band mask only a path along the
    band's edge gains mass: expected on the imperfect reads at band 50 alone (at least 1 % of their columns; measured 50 %, and
    0 % on the five other sets, which is recorded, not asserted). g * (x * x) differs from (g * x) * x in last bits only -- far
    inside every bound on the read sets, where it must move nothing (measured: at most 4.5e-4 of a bound) -- so it is held bit
    for bit against a lattice of the test's own, where 4 of 9 columns differ."""
    if wrong == "square_first":
        lpm, lpe, x = slc.grouping_lattice()
        a, b = slc.sums(lpm, lpe, x), slc.sums(lpm, lpe, x, wrong)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        differ = int((a[2] != b[2]).sum())
        print(f"square_first: {differ} of {len(a[2])} columns of the grouping lattice differ in sumsq")
        assert differ >= 2
        third = np.exp(np.log(1.0 / 3.0))
        g = third + third
        assert np.array_equal(a[2], np.array([(g * v) * v for v in x[:len(a[2])]]))   # the definition's grouping, one term each
        for name in slc.NAMES:
            assert _moved(yards(name)[0], wrong) == 0.0
        return
    for name in slc.NAMES:
        share = float(np.mean([_moved(y, wrong) for y in yards(name)[:2]]))
        print(f"{wrong} on {name}: {100 * share:.1f} % of the columns leave a bound")
        if wrong == "no_band_mask":
            if name == "imperfect_band50":
                assert share >= 0.01, (wrong, name, share)
        else:
            assert share >= 0.5, (wrong, name, share)


def test_mutations_can_fail(yards):
    """the unmutated yardstick against itself differs by nothing: the comparison above is not vacuous"""
    y = yards("imperfect_band50")[0]
    a, b = y.at(), slc.sums(y.lpm, y.lpe, y.signal, None, False, y.window)
    assert all(np.array_equal(a[k], b[k]) for k in range(6))
    assert _moved(y, None) == 0.0
