"""GPU (-m gpu): posterior-weighted per-base levels (Aligner.set_soft_levels, soft_level_kernels.hpp). Whole reads through every
place a lattice lives -- the separate layout (plain and certified reads), the in-place layout, a page-starved pool, the
banded-lattice kernel -- against the NumPy restatement over the CPU oracle's lattices (tests/soft_level_cases.py): every column of
every read within the bounds it derives from the float log-posteriors the device reads, no column left out; pooled per k-mer the
sums are Oracle.train's, and the weights of a read sum to T - 1. A ticket and a second run return the same bits; switching the
phase on moves nothing else; with rescaling the sums belong to the last pass's signal; every row the command line writes carries
read(i)'s three values for the same preprocessed reads."""
import ctypes as C
import os

import numpy as np
import pytest

import border_confidence_cases as bcc
import soft_level_cases as slc
from conftest import model_for
from dynamont_amd import Aligner, _native, synth, zstd_io
from dynamont_amd._dynamont import soft_level_columns
from dynamont_amd.segmentation import segment as seg

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

COLS = ("soft_weight", "soft_sum", "soft_sumsq")


@pytest.fixture(scope="module")
def sets(models):
    return slc.read_sets(models)


@pytest.fixture(scope="module")
def yards(models, sets, oracle_built):
    cache = {}
    return lambda name: slc.make_yards(models, sets, name, cache)


def run(model, pore, band, reads, on=True, budget=None, rescale=0, extras=False):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    if rescale:
        al.set_rescale(rescale)
    if extras:
        al.set_event_stats(True)
        al.set_segment_scores(8)
        al.set_kmer_summary(True)
        al.set_band_margin(True)
    al.set_soft_levels(on)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        b.align(True)
        res = b.fetch()
        tm = b.timing()
    al.close()
    if not on:
        assert all(getattr(res, c) is None for c in COLS) and "soft_dwell" not in res.read(0)
    return res, tm


def check(res, ys, what):
    """every column of every read against the yardstick; the pooled sums against Oracle.train; the weights against T - 1"""
    assert (res.status[:len(ys)] == 0).all(), (what, res.status)
    assert all(getattr(res, c).dtype == np.float64 for c in COLS)
    worst = np.zeros(3)
    for i, y in enumerate(ys):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        assert m == y.N - 1 and np.array_equal(res.signal_positions[a:a + m], y.res["signal_positions"]), (what, i)
        got = [getattr(res, c)[a:a + m] for c in COLS]
        worst = np.maximum(worst, slc.check_device(y, *got, f"{what} read {i}"))
        tw, t1, t2 = y.at()[3:]
        total = float(np.cumsum(got[0])[-1])
        assert abs(total - (y.T - 1)) <= float(tw.sum()), (what, i, total, y.T - 1)
        tr = y.orc.train(y.signal, y.seq, dense=False)
        K = y.orc.num_kmers
        for mine, key, tol in zip(y.pooled(got, K), ("weight", "sum", "sumsq"), y.pooled((tw, t1, t2), K)):
            err = np.abs(mine - tr[key])
            assert (err <= tol).all(), (what, i, key, float(err.max()))
    print(f"{what}: worst weight / sum / sumsq error {worst[0]:.3f} / {worst[1]:.3f} / {worst[2]:.3f} of its bound")
    return worst


def same_bits(a, b, cols, what=""):
    m = int(a.seg_offsets[-1])
    for c in cols:
        x, y = getattr(a, c), getattr(b, c)
        k = m if x.shape[0] >= m and c not in ("Z", "status") else x.shape[0]
        assert np.array_equal(np.ascontiguousarray(x[:k]).view(np.uint8), np.ascontiguousarray(y[:k]).view(np.uint8)), (what, c)


SEGMENTS = ("status", "Z", "n_segments", "seg_offsets", "signal_positions", "sequence_positions", "probabilities")
RIDERS = ("level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity", "band_margin_low", "band_margin_high",
          "band_edge_rows")


# ---- 1. separate layout, plain and certified reads; 2. band 50; 3. slot wrapping ---------------------------------------------------
@pytest.mark.parametrize("name", slc.NAMES)
def test_separate_layout_every_read_set(models, sets, yards, name):
    """plain: rna004 reads, the plain launch; imperfect: rna002 reads (a structural tie at the read's start), the launch that
    carries both arithmetic flavours; band 50: most of a lane's slots hold no column, and on the imperfect reads the path runs
    along the band's edge; long: 693 lattice columns, so the band slots wrap and a lane hands a finished column over."""
    key, pore, band, reads = sets[name]
    ys = yards(name)
    if name.startswith("long"):
        assert all(y.N > 448 for y in ys)
    res, tm = run(models[key], pore, band, reads)
    assert tm["lp_inplace"] == 0 and tm["launches"] == 1
    if name.startswith("imperfect"):
        assert tm["reads_strict"] == len(reads)
    check(res, ys, f"{name} separate")
    d = res.read(1)
    a, m = int(res.seg_offsets[1]), int(res.n_segments[1])
    want = soft_level_columns(*(getattr(res, c)[a:a + m] for c in COLS))
    for key_, w in zip(("soft_dwell", "soft_mean", "soft_stdv"), want):
        assert np.array_equal(d[key_], w)
    assert (d["soft_dwell"] >= 1.0).all() and (d["soft_stdv"] > 0).all()


# ---- 4. in-place layout and a page-starved pool --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["inplace", "page_starved"])
@pytest.mark.parametrize("name", ["plain", "imperfect_band50", "long_band50"])
def test_inplace_layout_and_page_starved_pool(models, sets, yards, monkeypatch, name, path):
    key, pore, band, reads = sets[name]
    budget = None
    if path == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    else:
        # a read's lattice takes ~(448 * 8 + 56) bytes per row: room for a fifth of the batch, and for the longest read one and a
        # half times over
        lens = sorted((len(r.signal) for r in reads), reverse=True)
        budget = int(max(0.2 * sum(lens), 1.5 * lens[0]) * (448 * 8 + 56))
    res, tm = run(models[key], pore, band, reads, budget=budget)
    off, _ = run(models[key], pore, band, reads, on=False, budget=budget)
    if path == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
        assert tm["lp_inplace"] == 1
        if name.startswith("imperfect"):
            assert tm["reads_strict"] == len(reads)                 # in place AND both flavours: k_read_queue<JOB_ALIGN_INPLACE | JOB_SOFT, true>
    check(res, yards(name), f"{name} {path}")
    same_bits(res, off, SEGMENTS, path)


# two of the six "plain" reads carry a tie by chance (dyn_tie_rows), so every batch above takes the launch with both arithmetic
# flavours; these four carry none
PLAIN_WITHOUT_A_TIE = (1, 2, 4, 5)


@pytest.mark.parametrize("layout", ["separate", "inplace"])
def test_launch_without_a_certified_read(models, sets, yards, monkeypatch, layout):
    """k_read_queue<JOB_ALIGN | JOB_SOFT, false> and <JOB_ALIGN_INPLACE | JOB_SOFT, false>: a batch the tie rule flags no read of,
    held as the batches above are"""
    key, pore, band, reads = sets["plain"]
    reads, ys = [reads[i] for i in PLAIN_WITHOUT_A_TIE], [yards("plain")[i] for i in PLAIN_WITHOUT_A_TIE]
    if layout == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    res, tm = run(models[key], pore, band, reads)
    off, _ = run(models[key], pore, band, reads, on=False)
    if layout == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
    assert tm["lp_inplace"] == (1 if layout == "inplace" else 0) and tm["launches"] == 1 and tm["reads_strict"] == 0
    check(res, ys, f"plain without a tie, {layout}")
    same_bits(res, off, SEGMENTS, layout)


# ---- 5. the banded-lattice kernel ------------------------------------------------------------------------------------------------
def test_banded_lattice_kernel(models, oracle_built):
    """one rna002 read of 600 bases at band = 600: half band 298, above the register sweeps' 223 (band_reads.hip)"""
    from oracle.pyoracle import Oracle
    reads = bcc.plain_reads(models["syn5"], "rna002", bcc.WIDE_SEED, 1, 600)
    assert min(600 // 2, (len(reads[0].sequence) - 5 + 2) // 2) == 298
    orc = Oracle(models["syn5"], synth.PORES["rna002"][0], 600)
    ys = [slc.Yard(orc, reads[0].signal, reads[0].sequence, 600)]
    res, _ = run(models["syn5"], "rna002", 600, reads)
    check(res, ys, "wide")
    same_bits(res, run(models["syn5"], "rna002", 600, reads, on=False)[0], SEGMENTS, "wide")


# ---- 6. reproducible, the same through a ticket, nothing else moves, the last pass's with rescaling ------------------------------
def test_runs_tickets_and_riders(models, sets):
    key, pore, band, reads = sets["plain"]
    first, _ = run(models[key], pore, band, reads, extras=True)
    again, _ = run(models[key], pore, band, reads, extras=True)
    same_bits(first, again, COLS, "second run")                              # two runs: identical bits
    off, _ = run(models[key], pore, band, reads, on=False, extras=True)
    same_bits(first, off, SEGMENTS + RIDERS, "switch on against off")        # no segment, Z, probability, level, score or margin moved
    al = Aligner(models[key], pore, band=band, device=0)
    al.set_soft_levels(True)
    t = al.align_async(*synth.pack_reads(reads), True)
    res = t.wait()
    same_bits(res, first, SEGMENTS + COLS, "ticket")                         # an asynchronous ticket: the bits of align_batch
    assert t.timing()["launches"] >= 1                                       # a launch of its own: no session
    m = int(res.seg_offsets[-1])
    w, s1, s2 = np.zeros(m + 5), np.zeros(m + 5), np.zeros(m + 5)
    p64 = lambda x: x.ctypes.data_as(_native.c_double_p)  # noqa: E731
    t.fetch_soft_levels(_native.DynSoftLevelOut(p64(w), p64(s1), p64(s2), m + 5))
    assert np.array_equal(w[:m], res.soft_weight[:m]) and np.array_equal(s2[:m], res.soft_sumsq[:m]) and not w[m:].any()
    with pytest.raises(ValueError, match="dyn_soft_level_out.capacity"):
        t.fetch_soft_levels(_native.DynSoftLevelOut(p64(w), p64(s1), p64(s2), m - 1))
    t.close()
    al.set_soft_levels(False)
    plain = al.align_async(*synth.pack_reads(reads), True)
    plain.wait()
    with pytest.raises(ValueError, match=r"without dyn_aligner_set_soft_levels\(a, 1\)"):
        plain.fetch_soft_levels(_native.DynSoftLevelOut(p64(w), p64(s1), p64(s2), m + 5))
    plain.close()
    al.close()


def test_with_rescaling_the_sums_belong_to_the_last_pass(models, sets, oracle_built):
    """set_rescale(2) on distorted signals (1.2 x + 0.3): the phase runs in the last pass only, over the signal that pass aligned
    (Batch.signals()). Held, every column, against the yardstick of the oracle on exactly that signal."""
    from oracle.pyoracle import Oracle
    key, pore, band, reads = sets["plain"]
    reads = reads[:3]
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    al = Aligner(models[key], pore, band=band, device=0)
    al.set_rescale(2)
    al.set_soft_levels(True)
    with al.batch(sig, seq) as b:
        b.align(True)
        res = b.fetch()
        x = b.signals()
    al.set_soft_levels(False)
    with al.batch(sig, seq) as b:
        b.align(True)
        only = b.fetch()
    al.close()
    same_bits(res, only, SEGMENTS + ("rescale_shift", "rescale_scale"), "rescale with the switch against without")
    off = np.concatenate([[0], np.cumsum([len(v) for v in sig])]).astype(np.int64)
    xs = [x[int(off[i]):int(off[i + 1])] for i in range(len(sig))]
    assert (res.status == 0).all() and (res.rescale_iters >= 1).all()
    assert all(not np.array_equal(a, s0) for a, s0 in zip(xs, sig))            # the signal the last pass aligned is not the input
    orc = Oracle(models[key], synth.PORES[pore][0], band)
    check(res, [slc.Yard(orc, xs[i], seq[i], band) for i in range(len(sig))], "rescale(2)")


# ---- 7. a failed read and a read of N = 2 --------------------------------------------------------------------------------------
def test_failed_read_and_two_column_read(models, sets, yards):
    key, pore, band, reads = sets["plain"]
    tiny = bcc.plain_reads(models[key], pore, 31, 1, 9)[0]                  # 9 bases at k = 9: N = 2, one output row
    failed = synth.SynthRead(reads[1].signal, reads[1].sequence[:40] + "N" + reads[1].sequence[41:])   # fails validation
    batch = [reads[0], failed, tiny, reads[2]]
    res, _ = run(models[key], pore, band, batch)
    assert res.status[1] != 0 and (res.status[[0, 2, 3]] == 0).all() and res.n_segments[2] == 1
    a = int(res.seg_offsets[2])
    assert abs(res.soft_weight[a] - len(tiny.signal)) <= 1e-6               # the one base there is owns every sample
    lo, hi = int(res.seg_offsets[1]), int(res.seg_offsets[2])
    for c in COLS:
        assert not getattr(res, c)[lo:hi].any()                             # rows of the failed read stay 0
    ys = yards("plain")
    for i, j in ((0, 0), (3, 2)):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        slc.check_device(ys[j], *(getattr(res, c)[a:a + m] for c in COLS), f"mixed batch read {i}")


# ---- 8. the refusals on the device path; the sink --------------------------------------------------------------------------------
def test_refusals(models, sets):
    key, pore, band, reads = sets["plain"]
    sig, seq = [r.signal for r in reads[:3]], [r.sequence for r in reads[:3]]
    al = Aligner(models[key], pore, device=0)
    d = np.zeros(4096)
    mk = lambda cap: _native.DynSoftLevelOut(*(d.ctypes.data_as(_native.c_double_p),) * 3, cap)  # noqa: E731
    with al.batch(sig, seq) as b:
        b.align(True)                          # switch off at submission
        al.set_soft_levels(True)
        with pytest.raises(ValueError, match="without dyn_aligner_set_soft_levels"):
            b.fetch_soft_levels(mk(4096))
        b.align(False)                         # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_soft_levels(mk(4096))
        b.train()
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_soft_levels(mk(4096))
        b.align(True)
        b.fetch_soft_levels(mk(4096))
        with pytest.raises(ValueError, match="capacity"):
            b.fetch_soft_levels(mk(3))
        soft = "dyn_aligner_set_soft_levels is on, which does not combine with "
        for on, off, word in ((lambda: al.set_border_confidence(8), lambda: al.set_border_confidence(0), "dyn_aligner_set_border_confidence"),
                              (lambda: al.set_posterior_samples(4, 1), lambda: al.set_posterior_samples(0), "dyn_aligner_set_posterior_samples"),
                              (lambda: al.set_border_interval(0.9), lambda: al.set_border_interval(0), "dyn_aligner_set_border_interval"),
                              (lambda: al.set_guide_rescue(4, 16), lambda: al.set_guide_rescue(0, 0), "dyn_aligner_set_guide_rescue")):
            on()
            with pytest.raises(ValueError, match="dyn_batch_align: " + soft + word):
                b.align(True)
            with pytest.raises(ValueError, match="dyn_batch_align_async: " + soft + word):
                al.align_async(*synth.pack_reads(reads[:3]), True)
            off()
        al.set_auto_guide(16)
        with pytest.raises(ValueError, match=soft + "dyn_aligner_set_auto_guide"):
            al.align_async(*synth.pack_reads(reads[:3]), True)
        al.set_auto_guide(0)
        b.align(True)                          # every other switch off again: accepted
    with pytest.raises(ValueError, match="carries a guide"):
        al.align_batch_auto(sig, seq, 16, 1)
    al.close()


def test_through_the_sink(models, sets, tmp_path):
    key, pore, band, reads = sets["plain"]
    reads = reads[:3]
    al = Aligner(models[key], pore, device=0)
    L = _native.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    assert L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1,
                                  _native.DYN_CSV_SOFT_LEVELS, C.byref(h), err, 1024) == 0, err.value
    sig, sig_off, seqs, seq_off = synth.pack_reads(reads)
    n = len(reads)
    rid = (C.c_char_p * n)(*[f"r{i}".encode() for i in range(n)])
    sid = (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)])
    starts = np.full(n, 100, dtype=np.int64)
    lengths = np.diff(np.asarray(sig_off).astype(np.int64)).astype(np.uint64)
    so = np.ascontiguousarray(seq_off, dtype=np.uint64)

    def submit(t):
        return L.dyn_csv_sink_submit(h, al._h, t._h, C.byref(t.result._c), n, seqs, so.ctypes.data_as(_native.c_u64_p), rid, sid,
                                     starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(_native.c_u64_p))

    lacking = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(lacking) == _native.DYN_ERR_INVALID_ARGUMENT
    assert "the soft levels (DYN_CSV_SOFT_LEVELS) and this ticket was submitted without dyn_aligner_set_soft_levels(a, 1)" in al.last_error()
    al.set_soft_levels(True)
    on = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(on) == 0
    assert L.dyn_csv_sink_wait(h, 1, -1) == 1
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    lines = zstd_io.decompress(open(tmp_path / "o.csv.zst", "rb").read()).split(b"\n")
    assert lines[0].endswith(b",polish,soft_dwell,soft_mean,soft_stdv")
    res = on.wait()
    assert len(lines) - 2 == int(res.n_segments.sum())
    dwell, mean, stdv = soft_level_columns(res.soft_weight, res.soft_sum, res.soft_sumsq)
    for j in (0, 1, int(res.n_segments[0]) - 1, int(res.n_segments[0])):
        assert b",".join(lines[1 + j].split(b",")[-3:]) == f"{dwell[j]:.6f},{mean[j]:.6f},{stdv[j]:.6f}".encode(), (j, lines[1 + j])
    lacking.close()
    on.close()
    al.close()


# ---- 9. the command line -------------------------------------------------------------------------------------------------------------
def _cli(model, pore, raw, bam, out, *extra):
    seg.main(["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", pore, "--model_path", model,
              "--batch-reads", "4", "-o", str(out)] + list(extra))
    data = open(str(out) + ".zst", "rb").read()
    errors = os.path.splitext(str(out))[0] + ".errors"
    return zstd_io.decompress(data).decode(), open(errors).read() if os.path.exists(errors) else ""


def re_fixed6(text):
    whole, _, frac = text.partition(".")
    return whole.lstrip("-").isdigit() and len(frac) == 6 and frac.isdigit()


def test_command_line(models, tmp_path):
    """dynamont-resquiggle --soft-levels on a small file: three more fields per row, everything before them the run without the
    flag, and the values those of read(i) for the same reads, row by row; preprocessing on the host and the Python listener
    write the same bytes; a combination the library refuses is refused through the command line too"""
    pore = "rna004"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(7511, 6, pore, mean, sd, (60, 160))
    raw, bam, _ = synth.write_dataset(str(tmp_path / "in"), "sl", reads, pore, seed=3, basecalls="tsv")
    plain, plain_err = _cli(model, pore, raw, bam, tmp_path / "plain.csv")
    text, err = _cli(model, pore, raw, bam, tmp_path / "sl.csv", "--soft-levels")
    assert err == plain_err
    b_lines, s_lines = plain.splitlines(), text.splitlines()
    assert s_lines[0] == b_lines[0] + ",soft_dwell,soft_mean,soft_stdv" and len(b_lines) == len(s_lines) > 100
    per_read = {}
    for b, s in zip(b_lines[1:], s_lines[1:]):
        f = s.split(",")
        assert ",".join(f[:-3]) == b                    # everything before the new fields: the run without the flag
        per_read.setdefault(f[0], []).append((int(f[2]), int(f[3]), float(f[-3]), f[-3:]))
    # every dwell is positive, and the dwell of most bases -- not of all -- is near the called one
    near = total = 0
    for rows in per_read.values():
        assert all(r[2] > 0 and float(r[3][2]) > 0 and all(re_fixed6(v) for v in r[3]) for r in rows)
        near += sum(abs(r[2] - (r[1] - r[0])) <= 0.5 for r in rows)
        total += len(rows)
    print(f"command line: {near} of {total} bases have a soft dwell within 0.5 samples of the called one")
    assert 0.5 * total <= near < total
    # ... and every row's three fields are read(i)'s: the reads the command line took, preprocessed as it preprocesses them
    # (generate_jobs, prepare_job: slice, shift, scale, Hampel; the basecall reversed behind the polyA pad), aligned through
    # Aligner with the switch on, and soft_dwell / soft_mean / soft_stdv of read(i) formatted as Python formats them
    jobs = list(seg.generate_jobs(os.path.dirname(raw), bam))
    prepared = [seg.prepare_job(job, True) for job in jobs]
    seg.close_raw_cache()
    assert sorted(job[6] for job in jobs) == sorted(per_read)
    al = Aligner(model, pore, device=0)
    al.set_soft_levels(True)
    res = al.align_batch([sig for sig, _ in prepared], [seq for _, seq in prepared], True)
    al.close()
    compared = 0
    for i, job in enumerate(jobs):
        d = res.read(i)
        rows = per_read[job[6]]
        assert len(rows) == len(d["soft_dwell"])
        first = min(r[0] for r in rows)                                     # the read's offset: the `start` column's unit
        at = {int(pos) + first: k for k, pos in enumerate(d["signal_positions"])}
        assert len(at) == len(rows)
        for r in rows:
            k = at[r[0]]
            assert r[3] == [f"{d['soft_dwell'][k]:.6f}", f"{d['soft_mean'][k]:.6f}", f"{d['soft_stdv'][k]:.6f}"], (job[6], k, r)
            compared += 1
    assert compared == len(s_lines) - 1
    # the other paths write the same bytes: preprocessing on the host, and the Python listener (which hands the same sums to the
    # same native formatter, so it adds the path, not a second derivation)
    for tag, extra in (("host", ["--host-preprocess"]), ("frames", ["--parallel-zstd-frames"])):
        other, other_err = _cli(model, pore, raw, bam, tmp_path / f"{tag}.csv", "--soft-levels", *extra)
        assert other == text and other_err == err, tag
    with pytest.raises((ValueError, SystemExit)):
        _cli(model, pore, raw, bam, tmp_path / "bad.csv", "--soft-levels", "--border-interval", "0.9")
