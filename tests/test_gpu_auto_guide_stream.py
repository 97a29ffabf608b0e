"""GPU (-m gpu): the self-guided band for asynchronous tickets (dyn_aligner_set_auto_guide, Aligner.set_auto_guide) and for
dynamont-resquiggle --guide-auto. A ticket submitted under the switch refines every read inside ONE launch, by the workgroup
that holds the read (k_band_reads<LiveGuideWindow, .., REFINE> in band_reads.hip). The yardstick is always the synchronous
``align_batch_auto(signals, sequences, half_width, refine)`` on the same handle -- the round scheme, a launch per round -- and
"equal" means: status, Z bits, the bytes of every row, guide_rounds, guide_converged and the final guides.
  1. the kernel where rounds differ (half width 4: reads of 2, 3 and 5 alignments in one ticket)
  2. stopping early: refine 2 and refine 1
  3. the three kernel shapes (64 x 1, 64 x 4, 256 x 16)
  4. a stream: six tickets in flight over two handles, the switch toggled between submissions, resident session on
  5. raw tickets (preprocessing on the device on both sides)
  6. the riders: event stats, segment scores, band margins, k-mer summary
  7. the two submission refusals, and a memory budget that refuses the longest read alone
  8. the command line
Yardsticks are computed once per module and left unchanged. No torch in this process."""
import os

import numpy as np
import pytest

import auto_guide_cases as ac
import guided_band_cases as gc
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd._dynamont import format_csv
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

NARROW = 4          # B = 11: at this half width the stalled reads need 2, 3 and 5 alignments
SHAPES = {16: "64 x 1, B = 35", 100: "64 x 4, B = 203", 130: "256 x 16, B = 263"}


def sig_seq(reads):
    return [r.signal for r in reads], [r.sequence for r in reads]


def packed(reads):
    return synth.pack_reads([synth.SynthRead(r.signal, r.sequence) for r in reads])


def assert_same_rows(x, y, ix=None, iy=None):
    """reads ix of x carry the bytes of reads iy of y (tests/test_gpu_auto_guide.py's, restated)"""
    ix = range(x.n) if ix is None else ix
    iy = range(y.n) if iy is None else iy
    for i, j in zip(ix, iy):
        assert x.status[i] == y.status[j] and x.n_segments[i] == y.n_segments[j], (i, j)
        assert np.float64(x.Z[i]).tobytes() == np.float64(y.Z[j]).tobytes(), (i, j)
        a, b, m = int(x.seg_offsets[i]), int(y.seg_offsets[j]), int(x.n_segments[i])
        for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
            assert getattr(x, col)[a:a + m].tobytes() == getattr(y, col)[b:b + m].tobytes(), (col, i, j)


def assert_equal(t, want, refine):
    """the completed ticket t against the yardstick (align_batch_auto(.., guides=True))"""
    res = t.wait()
    assert res.n == want.n
    assert_same_rows(res, want)
    for i in np.flatnonzero(want.status != 0):
        assert res.error(i) == want.error(i), i
    if refine == 1:
        assert res.guide_rounds is None and res.guide_converged is None
    else:
        assert res.guide_rounds.dtype == np.uint32 and res.guide_rounds.tolist() == want.guide_rounds.tolist()
        assert res.guide_converged.tolist() == want.guide_converged.tolist()
    got = t.guide()
    assert len(got) == len(want.guides)
    for i, (a, b) in enumerate(zip(got, want.guides)):
        assert a.dtype == np.int32 and np.array_equal(a, b), (i, np.flatnonzero(a != b)[:5].tolist())
    return res


def submit(al, reads, hw, refine):
    """one ticket under the switch; the switch is off again when this returns (it is sampled at submission)"""
    al.set_auto_guide(hw, refine)
    try:
        return al.align_async(*packed(reads))
    finally:
        al.set_auto_guide(0)


@pytest.fixture(scope="module")
def ctx(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    al = Aligner(models["syn5"], gc.PORE, band=gc.STALL_BAND)
    fam = gc.build_reads(mean, sd)
    c = dict(fam=fam, model=models["syn5"], al=al, edge=ac.edge_reads(*synth.code_order_table(mean, sd, gc.K, False)), yard={})
    c["sets"] = {"stalled": fam["stall"] + fam["stall_mv"], "shapes": fam["stall"] + fam["e"][:24]}
    c["sets"]["stream"] = fam["stall"] + fam["stall_mv"] + fam["e"][:24] + [c["edge"][k] for k in ("n2", "tight", "nan")]
    assert len(fam["stall"]) == 16 and len(fam["stall_mv"]) == 6

    def yard(name, hw, refine):
        """align_batch_auto over the named read set, once"""
        if (name, hw, refine) not in c["yard"]:
            c["yard"][name, hw, refine] = al.align_batch_auto(*sig_seq(c["sets"][name]), hw, refine, guides=True)
        return c["yard"][name, hw, refine]

    c["yardstick"] = yard
    yield c
    al.close()


# ---- 1. the refining kernel against the round scheme, where rounds differ -------------------------------------------------------
def test_reads_of_two_three_and_five_alignments_in_one_ticket(ctx):
    want = ctx["yardstick"]("stalled", NARROW, 8)
    rounds = want.guide_rounds.tolist()
    print("yardstick guide_rounds at half width %d: %s" % (NARROW, rounds))
    assert (want.status == 0).all() and want.guide_converged.tolist() == [1] * want.n
    assert sum(r >= 3 for r in rounds) >= 3 and sum(r >= 5 for r in rounds) >= 1 and min(rounds) == 2
    with submit(ctx["al"], ctx["sets"]["stalled"], NARROW, 8) as t:
        assert_equal(t, want, 8)
        assert t.timing()["launches"] == 1


# ---- 2. stopping early ----------------------------------------------------------------------------------------------------------
def test_refine_two_stops_the_open_reads_at_round_two(ctx):
    full = ctx["yardstick"]("stalled", NARROW, 8)
    want = ctx["yardstick"]("stalled", NARROW, 2)
    late = [i for i, r in enumerate(full.guide_rounds.tolist()) if r >= 3]
    assert len(late) == 5
    assert want.guide_rounds.tolist() == [2] * want.n
    assert [int(want.guide_converged[i]) for i in late] == [0] * len(late)
    with submit(ctx["al"], ctx["sets"]["stalled"], NARROW, 2) as t:
        res = assert_equal(t, want, 2)
        assert [int(res.guide_rounds[i]) for i in late] == [2] * len(late)
        assert [int(res.guide_converged[i]) for i in late] == [0] * len(late)


def test_refine_one_is_the_prepass_and_one_alignment(ctx):
    want = ctx["yardstick"]("stalled", NARROW, 1)
    with submit(ctx["al"], ctx["sets"]["stalled"], NARROW, 1) as t:
        res = assert_equal(t, want, 1)
        assert res.guide_rounds is None
    # the result object refilled by a plain ticket carries no counts either
    with ctx["al"].align_async(*packed(ctx["sets"]["stalled"]), True, out=res) as t:
        assert t.wait().guide_rounds is None
        with pytest.raises(ValueError, match="submitted without Aligner.set_auto_guide"):
            t.guide()


# ---- 3. the three shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", sorted(SHAPES))
def test_every_shape_of_the_refining_kernel(ctx, hw):
    want = ctx["yardstick"]("shapes", hw, 8)
    assert min(want.guide_rounds[:16]) >= 2 and (want.status == 0).all(), SHAPES[hw]
    with submit(ctx["al"], ctx["sets"]["shapes"], hw, 8) as t:
        assert_equal(t, want, 8)


# ---- 4. a stream ----------------------------------------------------------------------------------------------------------------
def same_segments(a, b):
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "probabilities"):
        assert np.array_equal(getattr(a, col)[:m].view(np.uint64), getattr(b, col)[:m].view(np.uint64)), col


def test_guided_and_plain_tickets_alternate_in_flight(ctx, models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(7600 + j, 600, "rna004", mean, sd, (60, 120)) for j in range(2)]
    never = Aligner(models["syn9"], "rna004", device=0)                     # a handle that never turned the switch on
    base = [never.align_batch(*sig_seq(reads), True) for reads in data]
    never.close()
    al9 = Aligner(models["syn9"], "rna004", device=0)                       # guided and plain tickets alternate on this one
    al5 = ctx["al"]                                                         # ... and the committed families run beside them
    sub = [reads[:32] for reads in data]
    yard9 = [al9.align_batch_auto(*sig_seq(s), 16, 8, guides=True) for s in sub]
    yard5 = {hw: ctx["yardstick"]("stream", hw, 8) for hw in (NARROW, 16)}
    stream = ctx["sets"]["stream"]
    nan_at = len(stream) - 1
    # (handle, half width or 0, what) in submission order: six tickets in flight, the switch toggled between submissions
    plan = [(al9, 0, 0), (al9, 16, 0), (al5, NARROW, None), (al9, 0, 1), (al9, 16, 1), (al5, 16, None)]
    tickets = []
    for al, hw, k in plan:
        al.set_auto_guide(hw, 8)
        tickets.append(al.align_async(*packed(stream if k is None else sub[k] if hw else data[k]), True))
    al9.set_auto_guide(0)
    al5.set_auto_guide(0)
    try:
        for (al, hw, k), t in zip(plan, tickets):
            if hw == 0:
                res = t.wait()
                same_segments(res, base[k])
                assert res.guide_rounds is None
                assert t.timing()["launches"] == 0                          # published into the resident session (600 reads)
            else:
                want = yard5[hw] if k is None else yard9[k]
                res = assert_equal(t, want, 8)
                assert t.timing()["launches"] >= 1                          # a launch of its own: neither merged nor resident
                if k is None:                                               # the NaN read fails alone, as it does synchronously
                    assert res.status[nan_at] != 0 and res.error(nan_at) == want.error(nan_at)
                    assert (np.delete(res.status, nan_at) == 0).all()
    finally:
        for t in tickets:
            t.close()
    st = al9.session_stats()
    assert st["sessions"] >= 1 and st["aborted"] == 0
    al9.close()


# ---- 5. raw tickets -------------------------------------------------------------------------------------------------------------
def test_raw_ticket_equals_the_synchronous_raw_batch(ctx):
    reads = ctx["sets"]["stalled"]
    al = ctx["al"]
    rng = np.random.default_rng(8101)
    shift = rng.uniform(400, 500, len(reads))
    scale = rng.uniform(60, 90, len(reads))
    raw = [np.round(r.signal * sc + sh).astype(np.int16) for r, sh, sc in zip(reads, shift, scale)]
    seq = [r.sequence for r in reads]
    with al.batch_raw(raw, seq, shift, scale) as b:
        b.auto_guide(NARROW)
        b.set_guide_refine(8)
        b.align(True)
        want = b.fetch()
        want.guide_rounds, want.guide_converged = b.guide_rounds()
        want.guides = b.guide()
    assert (want.status == 0).all() and max(want.guide_rounds) >= 3
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in raw])
    seq_off = np.zeros(len(seq) + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seq])
    al.set_auto_guide(NARROW, 8)
    try:
        t = al.align_raw_async(np.concatenate(raw), off, shift, scale, "".join(seq).encode(), seq_off)
    finally:
        al.set_auto_guide(0)
    with t:
        assert_equal(t, want, 8)


# ---- 6. riders ------------------------------------------------------------------------------------------------------------------
def test_riders_follow_the_last_alignment_once(ctx):
    reads = ctx["sets"]["stalled"]
    al = ctx["al"]
    al.set_event_stats(True)
    al.set_segment_scores(8)
    al.set_band_margin(True)
    al.set_kmer_summary(True)
    try:
        al.reset_kmer_summary()
        want = al.align_batch_auto(*sig_seq(reads), NARROW, 8, guides=True)
        ks_want = al.kmer_summary()
        al.reset_kmer_summary()
        with submit(al, reads, NARROW, 8) as t:
            res = assert_equal(t, want, 8)
            ks_got = al.kmer_summary()
    finally:
        al.set_event_stats(False)
        al.set_segment_scores(0)
        al.set_band_margin(False)
        al.set_kmer_summary(False)
        al.reset_kmer_summary()
    assert max(want.guide_rounds) >= 5
    m = int(want.seg_offsets[-1])
    for col in ("level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity"):
        x, y = getattr(res, col), getattr(want, col)
        assert x is not None and y is not None and np.array_equal(x[:m].view(np.uint64), y[:m].view(np.uint64)), col
    for col in ("band_margin_low", "band_margin_high", "band_edge_rows"):
        x, y = getattr(res, col), getattr(want, col)
        assert x is not None and y is not None and np.array_equal(x, y), col
    assert ks_got["totals"] == ks_want["totals"] and ks_got["totals"]["reads_ok"] == len(reads)   # every read once
    for x, y in zip(ks_got["limbs"], ks_want["limbs"]):
        assert np.array_equal(x, y)


# ---- 7. refusals and budget -----------------------------------------------------------------------------------------------------
def test_submission_refusals(ctx):
    al = ctx["al"]
    reads = ctx["fam"]["stall"][:2]
    al.set_auto_guide(16, 8)
    try:
        for setter, arg, text in ((al.set_rescale, 2, r"dyn_aligner_set_rescale\(a, iters > 0\)"),
                                  (al.set_border_confidence, 4, r"dyn_aligner_set_border_confidence\(a, window > 0\)")):
            setter(arg)
            try:
                with pytest.raises(ValueError, match="dyn_batch_align_async: dyn_aligner_set_auto_guide is on, which does not combine with " + text):
                    al.align_async(*packed(reads), True)
                with al.align_async(*packed(reads), False) as t:          # a Z-only ticket is none of the switch's business
                    assert (t.wait().status == 0).all()
            finally:
                setter(0)
    finally:
        al.set_auto_guide(0)


def test_budget_refuses_the_longest_read_alone(ctx):
    al = ctx["al"]
    fam = ctx["fam"]
    hw = 25
    short = fam["b"][:4]
    long_read = fam["a"][int(np.argmax([len(r.signal) for r in fam["a"]]))]
    need_long = 25 * (len(long_read.signal) + 1) * (2 * hw + 3)
    need_short = max(25 * (len(r.signal) + 1) * (2 * hw + 3) for r in short)
    assert need_short * 2 < need_long
    mix = short[:2] + [long_read] + short[2:]
    al.set_mem_budget(need_long - 4096)
    try:
        want = al.align_batch_auto(*sig_seq(mix), hw, 8, guides=True)
        with submit(al, mix, hw, 8) as t:
            res = assert_equal(t, want, 8)
    finally:
        al.set_mem_budget(0)
    assert res.status.tolist() == [0, 0, 8, 0, 0] and res.error(2) == "Read too large for the device memory budget"
    assert res.guide_rounds[2] == 0


# ---- 8. the command line --------------------------------------------------------------------------------------------------------
def test_resquiggle_guide_auto(ctx, tmp_path, capfd):
    import uuid
    reads = ctx["fam"]["stall"]
    lead, seed, hw = 37, 5, gc.STALL_HALF_WIDTH
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "gs", [synth.SynthRead(r.signal, r.sequence) for r in reads], gc.PORE,
                                             seed=seed, lead=lead, container="pod5", basecalls="bam")

    def run(name, *, batch_reads=5, host=False, guide=True, report=""):
        out = str(tmp_path / (name + ".csv.zst"))
        capfd.readouterr()
        seg.segment(os.path.dirname(raw), bam, 1, out, ctx["model"], gc.PORE, "basic", minq=0.0, device=0, batch_reads=batch_reads,
                    host_preprocess=host, band=gc.STALL_BAND, band_report=report, guide_auto=hw if guide else 0, guide_rounds=8)
        return zstd_io.decompress(open(out, "rb").read()).decode(), capfd.readouterr().err

    text, err = run("host", host=True)
    # the API on the signals the command aligns (normalised, Hampel-filtered) and the sequences it hands the aligner
    sig, seq = [], []
    for x, s in expected:
        x = x.copy()
        hampel(x)
        sig.append(x)
        seq.append(s)
    al = ctx["al"]
    want = al.align_batch_auto(sig, seq, hw, 8)
    assert (want.status == 0).all()
    rids = [str(uuid.UUID(int=(seed << 64) | i)) for i in range(len(reads))]
    lines = text.splitlines()
    sid_of = {ln.split(",")[0]: ln.split(",")[1] for ln in lines[1:]}
    assert sorted(sid_of) == sorted(rids)
    buf, _, end = format_csv(al, want, seq, rids, [sid_of[r] for r in rids], [lead] * len(reads), [len(x) + lead for x in sig],
                             threads=2, compact=True)
    assert text.encode() == seg.CSV_HEADER + buf[:int(end[-1])].tobytes()
    assert "Reads aligned inside their own guide: 16; of those, reads whose guide did not converge within 8 alignments: %d" % \
        int((want.guide_converged == 0).sum()) in err
    # preprocessing on the device (the BAM-columns front end), and the whole run as one ticket: the same bytes again
    report = str(tmp_path / "band.tsv")
    assert run("device", report=report)[0] == text
    assert run("one", batch_reads=64)[0] == text
    # ... which a plain run at the handle's band does not write
    plain, plain_err = run("plain", guide=False)
    assert "their own guide" not in plain_err
    rows = lambda t: {rid: [ln for ln in t.splitlines()[1:] if ln.startswith(rid + ",")] for rid in rids}  # noqa: E731
    assert sum(rows(plain)[rid] != rows(text)[rid] for rid in rids) >= 1
    # --band-report: the margins against the guided window, 2 * HW wide
    rep = open(report).read().split("\n")
    assert rep[0] + "\n" == seg.BAND_REPORT_HEADER.decode() and len(rep) == len(reads) + 2
    assert {ln.split("\t")[3] for ln in rep[1:-1]} == {str(2 * hw)}
