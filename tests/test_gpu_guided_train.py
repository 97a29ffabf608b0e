"""GPU (-m gpu): guided-band training (Aligner.train_batch_guided / dyn_batch_train_guided, the TRAIN job of band_reads.hip under its guide window).
  a. a diagonal guide at half_width = min(band / 2, N / 2) is the oracle's train(): once per kernel shape and LDS regime (B =
     53, 67, 203, 255, 273 and 4 095, the raised LDS limit), Z with the oracle's bits
  b. any covering guide (diagonal, the true staircase, random steps of 0 .. 7) is oracle(band 4093).train
  c. the purpose: stalled reads at half width 16 around their true starts / a move table's guide equal the NumPy restatement
     (tests/guided_train_cases.py) and oracle(band 4093).train; train_batch at band 50 does not
  d. an infeasible guide costs its read alone; pooled statistics, host and device, are the ok reads' sums bit for bit
  e. 600 reads: the same bits run to run and with fewer arenas (workgroups reused across reads of different T, N)
  f. a raw batch (batch_raw + set_guide + train_guided) has the bits of the float batch; cells; the two refusals
  g. dynamont-train --guide-moves: the model written after one batch is train_batch_guided's under the test's own aggregation
The bar against the oracle is guided_train_cases.check_against_oracle. Oracle results are computed once per module. No torch in
this process."""
import ctypes
import os

import numpy as np
import pytest

import guided_band_cases as gc
import guided_train_cases as gt
from dynamont_amd import Aligner, bam_io, synth
from dynamont_amd import guide as G
from dynamont_amd.segmentation import train as train_cli
from dynamont_amd.segmentation.utils import hampel
from oracle.pyoracle import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

TRAIN_Z_MISMATCH = "Training failed: alignment scores do not match"
TODAYS_REFUSAL = "dyn_batch_train: the batch carries a guide .* training inside a guided band is not supported"
ARRAYS = ("Z", "status", "transitions", "em_count", "em_code", "em_mean", "em_stdev", "em_weight", "em_sum", "em_sumsq", "trans_counts")


@pytest.fixture(scope="module")
def ctx(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    c = dict(fam=gc.build_reads(mean, sd), model=models["syn5"], pore=synth.PORES[gc.PORE][0], oracles={}, ref={}, al={})

    def oracle(band):
        if band not in c["oracles"]:
            c["oracles"][band] = Oracle(c["model"], c["pore"], band)
        return c["oracles"][band]

    def ref(name, band, i):
        """oracle(band).train of read i of the family, once"""
        if (name, band, i) not in c["ref"]:
            r = c["fam"][name][i]
            c["ref"][name, band, i] = oracle(band).train(r.signal, r.sequence, dense=False)
        return c["ref"][name, band, i]

    def aligner(band):
        if band not in c["al"]:
            c["al"][band] = Aligner(c["model"], gc.PORE, band=band)
        return c["al"][band]

    c["oracle"], c["ref_of"], c["aligner"] = oracle, ref, aligner
    yield c
    for al in c["al"].values():
        al.close()


def sig_seq(reads):
    return [r.signal for r in reads], [r.sequence for r in reads]


def same_bits(x, y):
    return np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64)


def same_arrays(x, y):
    """every output array of two TrainBatchResults, bit for bit"""
    for name in ARRAYS:
        a, b = getattr(x, name), getattr(y, name)
        if not np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a, b.view(np.uint64) if b.dtype == np.float64 else b):
            return name
    return None


def held_to_the_oracle(res, reads, refs, what, z_bits=True, at=None):
    """at: the reads' indices in res (default: 0, 1, ...)"""
    worst = np.zeros(4)
    for i, r, ref in zip(at if at is not None else range(len(reads)), reads, refs):
        assert res.status[i] == 0, (what, i, res.error(i))
        if z_bits:
            assert same_bits(res.Z[i], ref["Z"]), (what, i, res.Z[i], ref["Z"])
        else:
            assert abs(res.Z[i] - ref["Z"]) <= gc.Z_RTOL * abs(ref["Z"]), (what, i, res.Z[i], ref["Z"])
        dev = gt.check_against_oracle(gt.device_codes(res, i), res.transitions[3 * i], res.transitions[3 * i + 2], ref, r.signal, (what, i))
        worst = np.maximum(worst, dev)
    print("%-30s %2d reads: weight %.3g  sum %.3g  sumsq %.3g  |sum w - S| / S %.3g" % ((what, len(reads)) + tuple(worst)))


def model_as_ref(mo, num_kmers):
    w, s1, s2 = gt.dense(mo.codes, num_kmers)
    return dict(Z=mo.Z, weight=w, sum=s1, sumsq=s2, m1=mo.m1, e2=mo.e2)


def model_of(ctx, al, r, guide, hw):
    orc = ctx["oracle"](4093)
    km = orc.kmers(r.sequence)
    mean, sd = orc.table()
    assert al.info.log_e1 == 0.0
    return gt.model_train(r.signal, km, mean[km], sd[km], float(al.info.log_m1), float(al.info.log_e2), guide, hw)


# ---- a ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hw,band", [("a", 25, 50), ("a", 32, 64), ("a", 100, 200), ("a", 126, 252), ("a2", 135, 270)])
def test_diagonal_guide_is_the_oracles_train(ctx, name, hw, band):
    """B = 53 (one column per lane), 67, 203 and 255 (64 lanes x up to four columns, ragged last lane), 273 (256 threads)"""
    fam = ctx["fam"][name]
    floor = {25: 51, 32: 201, 100: 201, 126: 252, 135: 271}[hw]      # the oracle clamps its half band to N / 2, the guide does not
    idx = [i for i, r in enumerate(fam) if r.n_kmers + 1 >= floor][:8]
    assert len(idx) >= (8 if name == "a" else 4) and all((fam[i].n_kmers + 1) // 2 >= hw for i in idx)
    reads = [fam[i] for i in idx]
    res = ctx["aligner"](50).train_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], hw)
    held_to_the_oracle(res, reads, [ctx["ref_of"](name, band, i) for i in idx], "%s at half width %d" % (name, hw))


def test_the_widest_window(ctx):
    """half width 2046, B = 4095: 16 columns per thread, the raised dynamic-LDS limit, 16 B per cell of arena"""
    r = ctx["fam"]["w"][0]
    assert (r.n_kmers + 1) // 2 >= 2046
    with ctx["aligner"](50).batch(*sig_seq([r])) as b:
        b.set_guide(gc.diagonal(r), 2046)
        b.train_guided()
        res = b.fetch_train()
        assert b.arena_bytes() == (16 * (len(r.signal) + 1) * 4095 + 255) // 256 * 256
    held_to_the_oracle(res, [r], [ctx["ref_of"]("w", 4093, 0)], "w at half width 2046")


# ---- b ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["diagonal", "true", "random"])
def test_any_covering_guide_is_the_oracle_at_the_widest_band(ctx, kind):
    reads = ctx["fam"]["b"]
    assert len(reads) == 16 and all(gc.covers(len(r.signal) + 1, r.n_kmers + 1) for r in reads)
    hw = max(r.n_kmers + 1 for r in reads)
    rng = np.random.default_rng(11)
    guides = [gc.diagonal(r) if kind == "diagonal" else gc.true_guide(r) if kind == "true"
              else gc.random_staircase(rng, len(r.signal), r.n_kmers + 1) for r in reads]
    if kind == "random":
        assert max(int(np.diff(g).max()) for g in guides) >= 6      # shifts far above 1
    res = ctx["aligner"](50).train_batch_guided(*sig_seq(reads), guides, hw)
    held_to_the_oracle(res, reads, [ctx["ref_of"]("b", 4093, i) for i in range(16)], "b, " + kind)


# ---- c ---------------------------------------------------------------------------------------------------------------------
def test_the_purpose(ctx):
    al = ctx["aligner"](gc.STALL_BAND)
    K = al.num_kmers
    hw = gc.STALL_HALF_WIDTH
    stall, stall_mv = ctx["fam"]["stall"], ctx["fam"]["stall_mv"]
    assert len(stall) == 16 and len(stall_mv) == 6
    mv_guides = []
    for r in stall_mv:
        mv, ts = gc.moves_over_starts(r.starts, len(r.signal), stride=5)
        mv_guides.append(G.guide_from_moves(mv, len(r.signal), len(r.sequence), gc.K, ts=ts))
    for name, reads, guides in (("stall", stall, [gc.true_guide(r) for r in stall]), ("stall_mv", stall_mv, mv_guides)):
        res = al.train_batch_guided(*sig_seq(reads), guides, hw)
        models = [model_as_ref(model_of(ctx, al, r, g, hw), K) for r, g in zip(reads, guides)]
        held_to_the_oracle(res, reads, models, name + " vs the restatement", z_bits=False)
        held_to_the_oracle(res, reads, [ctx["ref_of"](name, 4093, i) for i in range(len(reads))], name + " vs oracle(4093)", z_bits=False)
    plain = al.train_batch(*sig_seq(stall))
    shifts = []
    for i, r in enumerate(stall):
        assert plain.status[i] == 0
        w50 = gt.dense(gt.device_codes(plain, i), K)[0]
        shifts.append(gt.weight_shift(w50, ctx["ref_of"]("stall", 4093, i)["weight"], len(r.signal)))
    print("train_batch at band 50: sum |w - w_4093| / S between %.3f and %.3f" % (min(shifts), max(shifts)))
    assert min(shifts) > 0.05, shifts


# ---- d ---------------------------------------------------------------------------------------------------------------------
def test_an_infeasible_guide_costs_its_read_only_and_the_pooled_sums(ctx):
    fam = ctx["fam"]["a"]
    jump = next(i for i, r in enumerate(fam) if r.n_kmers + 1 >= 140)          # room for a jump of 2 hw + 4 columns
    idx = [i for i in range(len(fam)) if i != jump][:4]
    idx.insert(2, jump)
    hw = 25
    reads = [fam[i] for i in idx]
    guides = [gc.diagonal(r) for r in reads]
    g = guides[2].copy()
    s = len(g) // 4
    g[s:] = np.maximum(g[s:], g[s - 1] + 2 * hw + 4)                             # consecutive windows are disjoint
    assert g.max() <= reads[2].n_kmers and g[s] - g[s - 1] == 2 * hw + 4
    guides[2] = g.astype(np.int32)
    al = ctx["aligner"](50)
    K = al.num_kmers
    four = al.train_batch_guided(*sig_seq(reads[:2] + reads[3:]), guides[:2] + guides[3:], hw)
    with al.batch(*sig_seq(reads)) as b:
        b.set_guide(np.concatenate(guides), hw)
        b.train_guided()
        five = b.fetch_train(pooled=True)
        ptr, cnt = b.device_pooled()
        dev = np.empty(cnt)
        hip = ctypes.CDLL("libamdhip64.so.7")                                  # the runtime this process has already loaded
        assert hip.hipMemcpy(ctypes.c_void_p(dev.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(cnt * 8), 2) == 0
    assert five.status.tolist() == [0, 0, 6, 0, 0] and five.error(2) == TRAIN_Z_MISMATCH and five.em_count[2] == 0
    assert five.transitions[6:9].tolist() == [0.0, 0.0, 0.0]
    pooled = np.zeros(3 * K)
    for k5, k4 in ((0, 0), (1, 1), (3, 2), (4, 3)):
        assert four.status[k4] == 0 and same_bits(five.Z[k5], four.Z[k4])
        c5, c4 = gt.device_codes(five, k5), gt.device_codes(four, k4)
        assert list(c5) == list(c4)
        for code in c5:
            assert all(same_bits(x, y) for x, y in zip(c5[code], c4[code])), (k5, code)
            for j in range(3):
                pooled[j * K + code] += c5[code][j]                             # the ok reads in input order
        assert np.array_equal(five.transitions[3 * k5:3 * k5 + 3], four.transitions[3 * k4:3 * k4 + 3])
    assert np.array_equal(five.pooled.view(np.uint64), pooled.view(np.uint64))
    assert cnt == 3 * K and np.array_equal(dev.view(np.uint64), five.pooled.view(np.uint64))


# ---- e ---------------------------------------------------------------------------------------------------------------------
def test_more_reads_than_workgroups_same_bits(ctx):
    reads = ctx["fam"]["e"]
    assert len(reads) == 600 and len({len(r.signal) for r in reads}) > 200
    al = ctx["aligner"](16)
    K = al.num_kmers
    hw = 8                                                                     # B = 19: the 64-thread shape
    flat = np.concatenate([gc.diagonal(r) for r in reads])

    def run(budget):
        al.set_mem_budget(budget)
        try:
            with al.batch(*sig_seq(reads)) as b:
                b.set_guide(flat, hw)
                b.train_guided()
                return b.fetch_train(pooled=True), b.arena_bytes()
        finally:
            al.set_mem_budget(0)

    one_arena = (16 * max(len(r.signal) + 1 for r in reads) * (2 * hw + 3) + 255) // 256 * 256
    first, bytes_first = run(0)
    second, bytes_second = run(0)
    few, bytes_few = run(24 * one_arena + 4096)                                # arenas for 24 workgroups: each takes ~25 reads
    assert bytes_first == bytes_second and bytes_few == 24 * one_arena and bytes_first >= 4 * bytes_few
    assert (first.status == 0).all()
    assert same_arrays(first, second) is None and same_arrays(first, few) is None
    assert np.array_equal(first.pooled.view(np.uint64), few.pooled.view(np.uint64))
    sub = list(range(0, 600, 25))
    models = [model_as_ref(model_of(ctx, al, reads[i], gc.diagonal(reads[i]), hw), K) for i in sub]
    held_to_the_oracle(first, [reads[i] for i in sub], models, "e, every 25th vs the restatement", z_bits=False, at=sub)


# ---- f ---------------------------------------------------------------------------------------------------------------------
def test_raw_batch_cells_and_refusals(ctx):
    reads = ctx["fam"]["b"][:4]
    al = ctx["aligner"](50)
    hw = 12
    guides = [gc.true_guide(r) for r in reads]
    flat = np.concatenate(guides)
    shift, scale = 90.0, 15.0
    raws = [(r.signal * scale + shift).astype(np.float32) for r in reads]
    host = []
    for x in raws:                                                             # the front end's host preprocessing, float32
        s = x.copy()
        s -= shift
        s /= scale
        hampel(s, 7, 5.0)
        host.append(s)
    seqs = [r.sequence for r in reads]
    want = al.train_batch_guided(host, seqs, guides, hw)
    with al.batch_raw(raws, seqs, [shift] * 4, [scale] * 4, window=7, n_sigmas=5.0, f32=True) as b:
        with pytest.raises(ValueError, match="dyn_batch_train_guided: the batch carries no guide"):
            b.train_guided()
        b.set_guide(flat, hw)
        with pytest.raises(ValueError, match=TODAYS_REFUSAL):
            b.train()
        b.train_guided()
        got = b.fetch_train()
        assert b.timing()["cells"] == sum((len(r.signal) + 1) * (2 * hw + 1) for r in reads)
        assert b.arena_bytes() == 4 * ((16 * max(len(r.signal) + 1 for r in reads) * (2 * hw + 3) + 255) // 256 * 256)
    assert (want.status == 0).all() and same_arrays(got, want) is None


# ---- g ---------------------------------------------------------------------------------------------------------------------
def _m_step(pooled, cur_mean, cur_sd):
    """the pooled M-step, restated: the test's own aggregation"""
    K = cur_mean.size
    w, s1, s2 = pooled[:K], pooled[K:2 * K], pooled[2 * K:]
    hit = w > 0
    mean, sd = cur_mean.copy(), cur_sd.copy()
    mean[hit] = s1[hit] / w[hit]
    sd[hit] = np.sqrt(np.maximum(s2[hit] / w[hit] - mean[hit] ** 2, 1e-12))
    return mean, sd


@pytest.fixture(scope="module")
def cli_data(tmp_path_factory, models):
    """seven stalled reads at dwell 9 whose signal begins where their move table does (the ten samples the table of
    gc.moves_over_starts lies ahead of the first k-mer are kept), the third without an mv tag"""
    _, mean, sd = synth.read_model_file(models["syn5"])
    mean_code, sd_code = synth.code_order_table(mean, sd, gc.K, False)
    rng = np.random.default_rng(7101)
    data = str(tmp_path_factory.mktemp("guided_train_cli"))
    reads, moves = [], []
    for _ in range(7):
        r = gc.make_read(rng, mean_code, sd_code, int(rng.integers(60, 121)), 9.0, stall=float(rng.uniform(0.3, 0.5)))
        mv, ts = gc.moves_over_starts(r.starts, len(r.signal), stride=5)
        lead = np.repeat(r.signal[:1], -ts) + 0.01 * rng.standard_normal(-ts)
        reads.append(synth.SynthRead(np.concatenate([lead, r.signal]), r.sequence))
        moves.append(mv)
    _, bam, _ = synth.write_dataset(data, "gt", reads, gc.PORE, seed=5, basecalls="bam")
    recs = []
    for i, rec in enumerate(bam_io.iter_bam(bam)):
        tags = {t: rec.get_tag(t) for t in ("qs", "ns", "ts", "fn", "sm", "sd")}
        if i != 2:
            tags["mv"] = moves[i]
        recs.append((rec.query_name, rec.query_sequence, tags))
    out = os.path.join(data, "gt_mv.bam")
    bam_io.write_bam(out, recs)
    return data, out


@pytest.mark.parametrize("host_preprocess", [False, True])
def test_cli_guide_moves(ctx, cli_data, tmp_path, capfd, host_preprocess):
    data, bam = cli_data
    hw = 16
    out = tmp_path / "out"
    out.mkdir()
    train_cli.train(data, bam, 6, 1, str(out / "params.csv"), "basic", ctx["model"], 1, gc.PORE, minq=0.0, device=0,
                    aggregate="pooled", host_preprocess=host_preprocess, guide_moves=hw)
    err = capfd.readouterr().err
    assert "Skipped reads without a move table (mv): 1" in err and "Skipped reads due to low quality: 0" in err
    items = [x for x in train_cli.read_items(data, bam, gc.PORE, 0.0, raw=False, guide_moves=hw, k=gc.K) if x != "noguide"]
    assert len(items) == 6 and all(len(x) == 4 for x in items)
    al = ctx["aligner"](400)
    cur_mean, cur_sd = al.model_table()
    try:
        sig, seq, gd = [x[0] for x in items], [x[1] for x in items], [x[3] for x in items]
        res = al.train_batch_guided(sig, seq, gd, hw, pooled=True)
        assert (res.status == 0).all()
        mean, sd = _m_step(res.pooled, cur_mean, cur_sd)
        _, fm, fs = synth.read_model_file(str(out / "trained_0_1.model"))
        fm, fs = synth.code_order_table(fm, fs, gc.K, False)
        assert np.array_equal(fm, mean) and np.array_equal(fs, sd) and not np.array_equal(mean, cur_mean)
        al.set_model(mean, sd)
        post = al.align_batch_guided(sig, seq, gd, hw, calc_probabilities=False)
        assert (post.status == 0).all()
        rows = (out / "params.csv").read_text().strip().split("\n")
        assert len(rows) == 2 and rows[1].split(",")[:3] == ["0", "1", "6"]
        assert float(rows[1].split(",")[6]) == float(np.mean(post.Z - res.Z))
    finally:
        al.set_model(cur_mean, cur_sd)


def test_cli_without_guide_moves_is_the_plain_run(ctx, cli_data, tmp_path, capfd):
    data, bam = cli_data
    out = tmp_path / "out"
    out.mkdir()
    train_cli.train(data, bam, 7, 1, str(out / "params.csv"), "basic", ctx["model"], 1, gc.PORE, minq=0.0, device=0,
                    aggregate="pooled", host_preprocess=True)
    assert "move table" not in capfd.readouterr().err
    items = list(train_cli.read_items(data, bam, gc.PORE, 0.0, raw=False))
    assert len(items) == 7 and all(len(x) == 3 for x in items)      # every read, the one without an mv tag included
    al = ctx["aligner"](400)
    cur_mean, cur_sd = al.model_table()
    res = al.train_batch([x[0] for x in items], [x[1] for x in items], pooled=True)
    mean, sd = _m_step(res.pooled, cur_mean, cur_sd)
    _, fm, fs = synth.read_model_file(str(out / "trained_0_1.model"))
    fm, fs = synth.code_order_table(fm, fs, gc.K, False)
    assert np.array_equal(fm, mean) and np.array_equal(fs, sd)
    assert sorted(os.listdir(out)) == ["params.csv", "trained_0_0.model", "trained_0_1.model"]
