"""GPU (-m gpu): the self-guided band (Batch.auto_guide / dyn_batch_auto_guide, auto_guide.hip; Batch.set_guide_refine /
dyn_batch_set_guide_refine; k_guide_refine in guided_band.hip, the alignments in band_reads.hip).
  1. k_auto_guide on descriptors of the test's own (tests/device_math/auto_guide.hip, built with the product's flags): every
     guide entry equals the g++ build of the same header in all three shapes, on the edge reads, on the empty range and with
     600 reads through a few workgroups
  2. through the product: the pre-pass and one alignment give oracle(band 4093)'s borders on the stalled reads
  3. refinement from the diagonal: rounds as the NumPy restatement counts them, borders of oracle(band 4093), the bytes of a
     by-hand loop of single calls
  4. what follows the traceback runs once per read
  5. train_batch_auto and dynamont-train --guide-auto
Oracle and model results are computed once per module. No torch in this process."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

import auto_guide_cases as ac
import guided_band_cases as gc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from dynamont_amd.segmentation import train as train_cli
from oracle.pyoracle import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

HW = gc.STALL_HALF_WIDTH
FILL = -7


@pytest.fixture(scope="module")
def ctx(models, tmp_path_factory):
    _, mean, sd = synth.read_model_file(models["syn5"])
    orc = Oracle(models["syn5"], synth.PORES[gc.PORE][0], 4093)
    al = Aligner(models["syn5"], gc.PORE, band=gc.STALL_BAND)
    assert al.info.log_e1 == 0.0
    c = dict(fam=gc.build_reads(mean, sd), model=models["syn5"], orc=orc, al=al, m1=float(al.info.log_m1), e2=float(al.info.log_e2),
             host=ac.build_host(tmp_path_factory.mktemp("ag_host")), edge=ac.edge_reads(*synth.code_order_table(mean, sd, gc.K, False)),
             truth={})

    def truth(name):
        """oracle(band 4093)'s borders of every read of the family, once"""
        if name not in c["truth"]:
            c["truth"][name] = [orc.align(r.signal, r.sequence, True)["signal_positions"].astype(np.int64) for r in c["fam"][name]]
        return c["truth"][name]

    c["truths"] = truth
    yield c
    al.close()


def params(ctx, r):
    """the emission entries of the read's lattice columns as the library holds them: -log(stdev) from the host's libm"""
    km = ctx["orc"].kmers(r.sequence)
    mean, sd = ctx["orc"].table()
    sd = np.ascontiguousarray(sd[km])
    return np.ascontiguousarray(mean[km]), sd, -np.array([math.log(v) for v in sd])


def host_guides(ctx, reads, hw):
    return [ac.host_guide(ctx["host"], r.signal, *params(ctx, r), ctx["m1"], ctx["e2"], hw) for r in reads]


def sig_seq(reads):
    return [r.signal for r in reads], [r.sequence for r in reads]


def borders(res, i):
    a = int(res.seg_offsets[i])
    return res.signal_positions[a:a + int(res.n_segments[i])].astype(np.int64)


def assert_same_rows(x, y, ix=None, iy=None):
    """reads ix of x carry the bytes of reads iy of y"""
    ix = range(x.n) if ix is None else ix
    iy = range(y.n) if iy is None else iy
    for i, j in zip(ix, iy):
        assert x.status[i] == y.status[j] and x.n_segments[i] == y.n_segments[j], (i, j)
        assert np.float64(x.Z[i]).tobytes() == np.float64(y.Z[j]).tobytes(), (i, j)
        a, b, m = int(x.seg_offsets[i]), int(y.seg_offsets[j]), int(x.n_segments[i])
        for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
            assert getattr(x, col)[a:a + m].tobytes() == getattr(y, col)[b:b + m].tobytes(), (col, i, j)


# ---- 1. the device harness ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("autoguide") / "libautoguide.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/auto_guide.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.ag_run.restype = C.c_int
    return lib


def run_harness(ctx, lib, reads, hw, n_groups, n_run=None):
    """the guides of `reads` (longest first, as the product queues them) from one launch; entries no read owns keep FILL"""
    order = sorted(range(len(reads)), key=lambda i: -len(reads[i].signal))
    par = [params(ctx, reads[i]) for i in order]
    T = np.array([len(reads[i].signal) + 1 for i in order], dtype=np.uint32)
    Ncol = np.array([reads[i].n_kmers + 1 for i in order], dtype=np.uint32)
    sig_off = np.concatenate([[0], np.cumsum(T - 1)]).astype(np.uint64)
    par_off = np.concatenate([[0], np.cumsum(Ncol - 1)]).astype(np.uint64)
    sig = np.concatenate([reads[i].signal for i in order] + [np.zeros(3)])          # three samples nobody owns
    mean, sd, nls = (np.ascontiguousarray(np.concatenate([p[k] for p in par])) for k in range(3))
    out = np.zeros(len(sig), dtype=np.int32)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.ag_run(C.c_int(len(order)), p(T), p(Ncol), p(sig_off), p(par_off), C.c_uint64(len(sig)), p(sig), C.c_uint64(len(mean)),
                   p(mean), p(sd), p(nls), C.c_int(hw), C.c_double(ctx["m1"]), C.c_double(ctx["e2"]),
                   C.c_int(len(order) if n_run is None else n_run), C.c_int(n_groups), C.c_int32(FILL), p(out), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert (out[int(sig_off[-1]):] == FILL).all()
    got = [None] * len(reads)
    for pos, i in enumerate(order):
        got[i] = out[int(sig_off[pos]):int(sig_off[pos + 1])]
    return got


def assert_guides(ctx, got, reads, hw, what):
    want = host_guides(ctx, reads, hw)
    for i, r in enumerate(reads):
        assert np.array_equal(got[i], want[i]), (what, i, np.flatnonzero(got[i] != want[i])[:5].tolist())
        assert ac.guide_invariants(got[i], r.n_kmers + 1) and int(got[i].max(initial=0)) <= r.n_kmers, (what, i)


def test_harness_one_column_per_lane(ctx, harness):
    """half width 16, B = 35: the 64 x 1 shape, the wave's butterfly alone; the edge reads ride along"""
    reads = ctx["fam"]["stall"] + list(ctx["edge"].values())
    e = ctx["edge"]
    assert e["n2"].n_kmers == 1 and len(e["tight"].signal) == 2 * e["tight"].n_kmers and np.isnan(e["nan"].signal).sum() == 1
    got = run_harness(ctx, harness, reads, HW, 5)
    assert_guides(ctx, got, reads, HW, "stall + edge")
    assert got[-2].tolist() == [(t + 1) // 2 for t in range(1, len(e["tight"].signal) + 1)]     # lo == hi in every row


def test_harness_many_reads_per_workgroup(ctx, harness):
    reads = ctx["fam"]["e"]
    assert len(reads) == 600
    assert_guides(ctx, run_harness(ctx, harness, reads, HW, 24), reads, HW, "e")


@pytest.mark.parametrize("hw", [100, 130])
def test_harness_wider_shapes(ctx, harness, hw):
    """half width 100, B = 203: 64 threads, up to four columns per lane; 130, B = 263: 256 threads, the cross-wave reduction"""
    reads = ctx["fam"]["a2"] + [ctx["edge"]["nan"], ctx["edge"]["n2"]]
    assert_guides(ctx, run_harness(ctx, harness, reads, hw, 3), reads, hw, "a2 at %d" % hw)


def test_harness_empty_range(ctx, harness):
    reads = ctx["fam"]["stall"][:2]
    for g in run_harness(ctx, harness, reads, HW, 2, n_run=0):
        assert (g == FILL).all()


# ---- 2. through the product: the pre-pass, then one alignment ----------------------------------------------------------------
def test_prepass_then_one_alignment_finds_the_oracles_borders(ctx):
    reads = ctx["fam"]["stall"]
    al = ctx["al"]
    with al.batch(*sig_seq(reads)) as b:
        b.auto_guide(HW)
        guides = b.guide()
        b.align(True)
        res = b.fetch()
        rounds, conv = b.guide_rounds()
        assert [g.tolist() for g in b.guide()] == [g.tolist() for g in guides]            # one alignment leaves the guide alone
        with pytest.raises(ValueError, match="dyn_batch_auto_guide: the batch has already run"):
            b.auto_guide(HW)
    want = host_guides(ctx, reads, HW)
    truth = ctx["truths"]("stall")
    for i in range(len(reads)):
        assert guides[i].dtype == np.int32 and np.array_equal(guides[i], want[i]), i
        assert res.status[i] == 0 and np.array_equal(borders(res, i), truth[i]), (i, res.error(i))
    assert rounds.tolist() == [1] * len(reads) and conv.tolist() == [0] * len(reads)
    assert_same_rows(res, al.align_batch_guided(*sig_seq(reads), guides, HW))               # the fetched guide, fed back by hand


def test_prepass_at_half_the_columns(ctx):
    """family b (covers() holds): a window of N / 2 columns on either side"""
    al = ctx["al"]
    truth = ctx["truths"]("b")
    for i, r in enumerate(ctx["fam"]["b"]):
        with al.batch(*sig_seq([r])) as b:
            b.auto_guide((r.n_kmers + 1) // 2)
            b.align(True)
            res = b.fetch()
        assert res.status[0] == 0 and np.array_equal(borders(res, 0), truth[i]), i


# ---- 3. refinement -----------------------------------------------------------------------------------------------------------
def path_guide(res, i, n_samples):
    """g'[s] = the called path's column at lattice row s + 1: the borders at or before it"""
    return np.searchsorted(borders(res, i) + 1, np.arange(1, n_samples + 1), side="right").astype(np.int32)


@pytest.fixture(scope="module")
def by_hand(ctx):
    """name -> per read (rounds, converged, final guide, (result, index) of the last alignment, results per round): a loop of
    single align_batch_guided calls from the diagonal, every round over every read still open"""
    out = {}
    al = ctx["al"]
    for name in ("stall", "stall_mv"):
        reads = ctx["fam"][name]
        guides = [gc.diagonal(r) for r in reads]
        state = [None] * len(reads)
        open_ = list(range(len(reads)))
        per_round = []
        for rnd in range(8):
            if not open_:
                break
            res = al.align_batch_guided(*sig_seq([reads[i] for i in open_]), [guides[i] for i in open_], HW)
            per_round.append((res, list(open_)))
            still = []
            for k, i in enumerate(open_):
                assert res.status[k] == 0
                g2 = path_guide(res, k, len(reads[i].signal))
                if np.array_equal(g2, guides[i]):
                    state[i] = (rnd + 1, 1, guides[i], (res, k))
                elif rnd == 7:
                    state[i] = (8, 0, guides[i], (res, k))
                else:
                    guides[i] = g2
                    still.append(i)
            open_ = still
        out[name] = (state, per_round)
    return out


@pytest.fixture(scope="module")
def model_rounds(ctx):
    """name -> the NumPy restatement's count of alignments per read"""
    out = {}
    for name in ("stall", "stall_mv"):
        out[name] = []
        for r in ctx["fam"][name]:
            mean, sd, _ = params(ctx, r)
            rounds, conv, _, _, _ = ac.refine(r.signal, mean, sd, ctx["m1"], ctx["e2"], gc.diagonal(r), HW, 8)
            assert conv == 1
            out[name].append(rounds)
    return out


@pytest.mark.parametrize("name", ["stall", "stall_mv"])
def test_refinement_from_the_diagonal(ctx, by_hand, model_rounds, name):
    reads = ctx["fam"][name]
    res = ctx["al"].align_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], HW, refine=8)
    truth = ctx["truths"](name)
    state, _ = by_hand[name]
    print("%s: guide_rounds %s" % (name, res.guide_rounds.tolist()))
    assert res.guide_converged.tolist() == [1] * len(reads)
    assert res.guide_rounds.tolist() == model_rounds[name] and max(model_rounds[name]) >= 3
    for i in range(len(reads)):
        assert res.status[i] == 0 and np.array_equal(borders(res, i), truth[i]), (i, res.error(i))
        rounds, conv, g, (hand, k) = state[i]
        assert (rounds, conv) == (int(res.guide_rounds[i]), 1) and np.array_equal(res.guides[i], g), i
        assert np.array_equal(borders(res, i), borders(hand, k)), i
        assert abs(res.Z[i] - hand.Z[k]) <= gc.Z_RTOL * abs(hand.Z[k]), i
        assert_same_rows(res, hand, [i], [k])


def test_refine_one_and_refine_two(ctx, by_hand, model_rounds):
    reads = ctx["fam"]["stall"]
    al = ctx["al"]
    guides = [gc.diagonal(r) for r in reads]
    plain = al.align_batch_guided(*sig_seq(reads), guides, HW)
    one = al.align_batch_guided(*sig_seq(reads), guides, HW, refine=1)
    assert_same_rows(one, plain)
    assert one.guide_rounds is None and plain.guide_rounds is None
    # a read that needs at least four alignments, stopped after two: round 2's result, not converged
    i = next(k for k, n in enumerate(model_rounds["stall"]) if n >= 4)
    two = al.align_batch_guided(*sig_seq([reads[i]]), [guides[i]], HW, refine=2)
    assert two.guide_rounds.tolist() == [2] and two.guide_converged.tolist() == [0] and two.status[0] == 0
    _, per_round = by_hand["stall"]
    hand, members = per_round[1]
    assert_same_rows(two, hand, [0], [members.index(i)])
    first, members0 = per_round[0]
    assert np.array_equal(two.guides[0], path_guide(first, members0.index(i), len(reads[i].signal)))   # the guide round 2 used


def test_converged_reads_are_left_alone(ctx):
    """reads whose guide reproduces itself in the first alignment, in one batch with reads that take several"""
    e, st = ctx["fam"]["e"][:24], ctx["fam"]["stall"]
    al = ctx["al"]
    settled = al.align_batch_guided(*sig_seq(e), [gc.diagonal(r) for r in e], HW, refine=8)
    assert settled.guide_converged.tolist() == [1] * len(e)
    single = al.align_batch_guided(*sig_seq(e), settled.guides, HW)
    mix = e[:12] + st + e[12:]
    guides = settled.guides[:12] + [gc.diagonal(r) for r in st] + settled.guides[12:]
    res = al.align_batch_guided(*sig_seq(mix), guides, HW, refine=8)
    at = list(range(12)) + list(range(12 + len(st), len(mix)))
    assert res.guide_rounds[at].tolist() == [1] * len(e) and res.guide_converged.tolist() == [1] * len(mix)
    assert min(res.guide_rounds[12:12 + len(st)]) >= 3
    assert_same_rows(res, single, at, range(len(e)))
    for k, i in enumerate(at):
        assert np.array_equal(res.guides[i], settled.guides[k])


# ---- 4. once-only follow-ups -------------------------------------------------------------------------------------------------
def test_followups_run_once_per_read(ctx):
    reads = ctx["fam"]["stall"]
    al = ctx["al"]
    al.set_event_stats(True)
    al.set_kmer_summary(True)
    try:
        al.reset_kmer_summary()
        refined = al.align_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], HW, refine=8)
        ks_refined = al.kmer_summary()
        al.reset_kmer_summary()
        once = al.align_batch_guided(*sig_seq(reads), refined.guides, HW)
        ks_once = al.kmer_summary()
    finally:
        al.set_event_stats(False)
        al.set_kmer_summary(False)
        al.reset_kmer_summary()
    assert min(refined.guide_rounds) >= 3
    assert_same_rows(refined, once)
    for col in ("level_mean", "level_stdv", "level_median"):
        x, y = getattr(refined, col), getattr(once, col)
        assert x is not None and y is not None and np.array_equal(x.view(np.uint64), y.view(np.uint64)), col
    assert ks_refined["totals"] == ks_once["totals"] and ks_once["totals"]["reads_ok"] == len(reads)
    for x, y in zip(ks_refined["limbs"], ks_once["limbs"]):
        assert np.array_equal(x, y)


# ---- 5. training -------------------------------------------------------------------------------------------------------------
def test_train_batch_auto(ctx):
    reads = ctx["fam"]["stall"]
    al = ctx["al"]
    auto = al.align_batch_auto(*sig_seq(reads), half_width=HW, refine=8, guides=True)
    truth = ctx["truths"]("stall")
    assert (auto.status == 0).all() and auto.guide_converged.tolist() == [1] * len(reads) and max(auto.guide_rounds) <= 8
    for i in range(len(reads)):
        assert np.array_equal(borders(auto, i), truth[i]), i
    tr = al.train_batch_auto(*sig_seq(reads), half_width=HW, refine=8, pooled=True)
    want = al.train_batch_guided(*sig_seq(reads), auto.guides, HW, pooled=True)
    assert tr.reads.tolist() == list(range(len(reads))) and tr.guide_converged.tolist() == [1] * len(reads)
    assert (want.status == 0).all() and np.array_equal(tr.status, want.status)
    for col in ("Z", "transitions", "pooled"):
        assert np.asarray(getattr(tr, col)).tobytes() == np.asarray(getattr(want, col)).tobytes(), col
    # a read that cannot align (three samples for nine k-mers) is left out, and the result says so
    short = np.zeros(3)
    tr2 = al.train_batch_auto([reads[0].signal, short, reads[1].signal], [reads[0].sequence, reads[1].sequence[:13], reads[1].sequence],
                              half_width=HW, refine=8)
    assert tr2.reads.tolist() == [0, 2] and np.asarray(tr2.Z).tobytes() == np.asarray(want.Z[:2]).tobytes()


def test_cli_guide_auto(ctx, tmp_path, capfd):
    """dynamont-train --guide-auto 16 on a BAM without a single mv tag: no read is skipped for it"""
    _, mean, sd = synth.read_model_file(ctx["model"])
    mean_code, sd_code = synth.code_order_table(mean, sd, gc.K, False)
    rng = np.random.default_rng(7102)
    reads = [gc.make_read(rng, mean_code, sd_code, int(rng.integers(60, 121)), 9.0, stall=float(rng.uniform(0.3, 0.5))) for _ in range(5)]
    data = str(tmp_path / "data")
    _, bam, _ = synth.write_dataset(data, "ag", [synth.SynthRead(r.signal, r.sequence) for r in reads], gc.PORE, seed=5, basecalls="bam")
    out = tmp_path / "out"
    out.mkdir()
    train_cli.train(data, bam, 5, 1, str(out / "params.csv"), "basic", ctx["model"], 1, gc.PORE, minq=0.0, device=0,
                    aggregate="pooled", host_preprocess=True, guide_auto=HW, guide_rounds=8)
    err = capfd.readouterr().err
    assert "move table" not in err and "Reads left out (no alignment inside their own guide): 0" in err
    assert "Reads whose guide did not converge within 8 alignments: 0" in err
    rows = (out / "params.csv").read_text().strip().split("\n")
    assert len(rows) == 2 and rows[1].split(",")[:3] == ["0", "1", "5"]                  # every read trained
    items = list(train_cli.read_items(data, bam, gc.PORE, 0.0, raw=False))
    assert len(items) == 5 and all(len(x) == 3 for x in items)
    al = Aligner(ctx["model"], gc.PORE, band=400)
    try:
        cur_mean, cur_sd = al.model_table()
        tr = al.train_batch_auto([x[0] for x in items], [x[1] for x in items], half_width=HW, refine=8, pooled=True)
        assert tr.reads.tolist() == list(range(5)) and (tr.status == 0).all()
        K = cur_mean.size
        w, s1, s2 = tr.pooled[:K], tr.pooled[K:2 * K], tr.pooled[2 * K:]
        hit = w > 0
        want_mean, want_sd = cur_mean.copy(), cur_sd.copy()
        want_mean[hit] = s1[hit] / w[hit]
        want_sd[hit] = np.sqrt(np.maximum(s2[hit] / w[hit] - want_mean[hit] ** 2, 1e-12))
    finally:
        al.close()
    _, fm, fs = synth.read_model_file(str(out / "trained_0_1.model"))
    fm, fs = synth.code_order_table(fm, fs, gc.K, False)
    assert np.array_equal(fm, want_mean) and np.array_equal(fs, want_sd) and not np.array_equal(want_mean, cur_mean)
