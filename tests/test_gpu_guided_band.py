"""GPU (-m gpu): the guided band (Aligner.align_batch_guided / dyn_batch_set_guide, band_reads.hip).
  a. a diagonal guide at half_width = min(band / 2, N / 2) is the reference's band: borders and Z bits of the CPU oracle, at one
     band column per lane (64 threads), at 67 / 203 / 255 band columns (64 threads, up to four columns per lane), at 273 (256
     threads, two columns per thread) and at 4 095 (16 per thread, the raised LDS limit); the Z-only job of each shape
  b. any guide that covers the lattice gives oracle(band 4093): diagonal, the true staircase, a random staircase with steps of
     0 .. 7 -- shifts above 1, windows clipped at both lattice borders
  c. the narrow off-diagonal window: stalled reads at half width 16 around their true starts (and around a move table's guide)
     against the NumPy restatement (tests/guided_band_cases.py) and oracle(band 4093); the plain band 50 does not find them
  d. infeasible guides cost their reads DYN_READ_Z_MISMATCH and nobody else anything
  e. 600 reads through far fewer workgroups: arena and LDS rows reused across reads of different sizes
  f. riders: event stats, segment scores, k-mer summary bit-equal to the unguided call; guided band margins exact
  g. the refusals that need a device, the memory budget, the cell count
  h. the kernel's two windows against each other: an unguided batch of wide reads (the diagonal window) equals, bit for bit, each
     read guided by the diagonal at its own half band; train to the bar of the wide band; the arena a job of wide reads allocates
Oracle results are computed once per module. No torch in this process."""
import numpy as np
import pytest

import guided_band_cases as gc
from dynamont_amd import Aligner, synth
from dynamont_amd import guide as G
from oracle.pyoracle import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

Z_MISMATCH = "Alignment failed: alignment scores do not match"


@pytest.fixture(scope="module")
def ctx(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    c = dict(fam=gc.build_reads(mean, sd), model=models["syn5"], pore=synth.PORES[gc.PORE][0], oracles={}, ref={}, al={})

    def oracle(band):
        if band not in c["oracles"]:
            c["oracles"][band] = Oracle(c["model"], c["pore"], band)
        return c["oracles"][band]

    def ref(name, band):
        """oracle(band).align of every read of the family, once"""
        if (name, band) not in c["ref"]:
            c["ref"][name, band] = [oracle(band).align(r.signal, r.sequence, True) for r in c["fam"][name]]
        return c["ref"][name, band]

    def aligner(band):
        if band not in c["al"]:
            c["al"][band] = Aligner(c["model"], gc.PORE, band=band)
        return c["al"][band]

    c["oracle"], c["refs"], c["aligner"] = oracle, ref, aligner
    yield c
    for al in c["al"].values():
        al.close()


def sig_seq(reads):
    return [r.signal for r in reads], [r.sequence for r in reads]


def borders(res, i):
    a = int(res.seg_offsets[i])
    return res.signal_positions[a:a + int(res.n_segments[i])].astype(np.int64)


def probs(res, i):
    a = int(res.seg_offsets[i])
    return res.probabilities[a:a + int(res.n_segments[i])]


def same_bits(x, y):
    return np.float64(x).view(np.uint64) == np.float64(y).view(np.uint64)


def assert_is_the_oracle(res, refs, what, reads=None, prob_tol=1e-6):
    for i, ref in enumerate(refs):
        assert res.status[i] == 0, (what, i, res.error(i))
        assert np.array_equal(borders(res, i), ref["signal_positions"].astype(np.int64)), (what, i)
        assert same_bits(res.Z[i], ref["Z"]), (what, i, res.Z[i], ref["Z"])
        if prob_tol is not None:
            assert np.abs(probs(res, i) - ref["probabilities"]).max() <= prob_tol, (what, i)


@pytest.fixture(scope="module")
def guided_a(ctx):
    """(a)'s guided result: shared with (d) and (f)"""
    reads = ctx["fam"]["a"]
    assert all(r.n_kmers + 1 >= 51 for r in reads)
    return ctx["aligner"](50).align_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], 25)


# ---- a ---------------------------------------------------------------------------------------------------------------------
def test_diagonal_guide_is_the_oracle_one_column_per_lane(ctx, guided_a):
    reads = ctx["fam"]["a"]
    refs = ctx["refs"]("a", 50)
    assert_is_the_oracle(guided_a, refs, "a")
    z = ctx["aligner"](50).align_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], 25, calc_probabilities=False)
    for i, ref in enumerate(refs):
        assert z.status[i] == 0 and same_bits(z.Z[i], ref["Z"]) and z.n_segments[i] == 0, i


def test_diagonal_guide_is_the_oracle_two_columns_per_thread(ctx):
    reads = ctx["fam"]["a2"]
    assert all(300 <= r.n_kmers <= 400 for r in reads)
    res = ctx["aligner"](270).align_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], 135)   # B = 273 > 256
    assert_is_the_oracle(res, ctx["refs"]("a2", 270), "a2")


def test_diagonal_guide_is_the_oracle_four_columns_per_lane(ctx):
    """65 <= B <= 256: the 64-thread shape with up to four band columns per lane (B = 203: lanes hold 4, 4, ..., 3 columns)"""
    reads = [r for r in ctx["fam"]["a"] if r.n_kmers + 1 >= 201]
    assert len(reads) >= 8
    refs = [ref for r, ref in zip(ctx["fam"]["a"], ctx["refs"]("a", 200)) if r.n_kmers + 1 >= 201]
    al = ctx["aligner"](200)
    guides = [gc.diagonal(r) for r in reads]
    assert_is_the_oracle(al.align_batch_guided(*sig_seq(reads), guides, 100), refs, "a at half width 100")
    z = al.align_batch_guided(*sig_seq(reads), guides, 100, calc_probabilities=False)
    for i, ref in enumerate(refs):
        assert z.status[i] == 0 and same_bits(z.Z[i], ref["Z"]) and z.n_segments[i] == 0, i
    # B = 67 (the first width of the shape: one lane in three holds a second column) and B = 255 (all but one lane hold four)
    for hw in (32, 126):
        sub = [r for r in reads if (r.n_kmers + 1) // 2 >= hw]      # the oracle clamps its half band to N / 2, the guide does not
        assert len(sub) >= 8
        res = al.align_batch_guided(*sig_seq(sub), [gc.diagonal(r) for r in sub], hw)
        orc_refs = [ctx["oracle"](2 * hw).align(r.signal, r.sequence, True) for r in sub]
        assert_is_the_oracle(res, orc_refs, "a at half width %d" % hw)


def test_the_widest_window(ctx):
    """half width 2046, B = 4095: 16 columns per thread, 130 KiB of dynamic LDS (the raised limit), against oracle(band 4093)"""
    r = ctx["fam"]["w"][0]
    assert (r.n_kmers + 1) // 2 >= 2046
    ref = ctx["refs"]("w", 4093)
    al = ctx["aligner"](4093)
    with al.batch(*sig_seq([r])) as b:
        b.set_guide(gc.diagonal(r), 2046)
        b.align(True)
        assert_is_the_oracle(b.fetch(), ref, "w")
        assert b.arena_bytes() == (25 * (len(r.signal) + 1) * 4095 + 255) // 256 * 256      # one workgroup's lattice
    with al.batch(*sig_seq([r])) as b:
        b.set_guide(gc.diagonal(r), 2046)
        b.align(False)
        z = b.fetch()
        assert z.status[0] == 0 and same_bits(z.Z[0], ref[0]["Z"]) and b.arena_bytes() == 0


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
    res = ctx["aligner"](50).align_batch_guided(*sig_seq(reads), guides, hw)
    assert_is_the_oracle(res, ctx["refs"]("b", 4093), kind, prob_tol=1e-6)


# ---- c ---------------------------------------------------------------------------------------------------------------------
def model_of(ctx, al, r, guide, hw):
    orc = ctx["oracle"](4093)
    km = orc.kmers(r.sequence)
    mean, sd = orc.table()
    assert al.info.log_e1 == 0.0
    return gc.model_align(r.signal, mean[km], sd[km], float(al.info.log_m1), float(al.info.log_e2), guide, hw)


def assert_is_the_model(res, i, mo, what):
    assert res.status[i] == 0 and mo.ok, (what, i, res.error(i))
    assert np.array_equal(borders(res, i), mo.signal_positions), (what, i)
    dev = abs(res.Z[i] - mo.Z) / abs(mo.Z)
    print("%s read %d: |Z - Z_model| / |Z_model| = %.3g" % (what, i, dev))
    assert dev <= gc.Z_RTOL, (what, i, dev)
    assert np.abs(probs(res, i) - mo.probabilities).max() <= 1e-6, (what, i)


def test_narrow_window_around_the_true_starts(ctx):
    reads = ctx["fam"]["stall"]
    al = ctx["aligner"](gc.STALL_BAND)
    guides = [gc.true_guide(r) for r in reads]
    res = al.align_batch_guided(*sig_seq(reads), guides, gc.STALL_HALF_WIDTH)
    plain = al.align_batch(*sig_seq(reads))
    truth = ctx["refs"]("stall", 4093)
    for i, r in enumerate(reads):
        assert_is_the_model(res, i, model_of(ctx, al, r, guides[i], gc.STALL_HALF_WIDTH), "stall")
        assert np.array_equal(borders(res, i), truth[i]["signal_positions"].astype(np.int64)), i
        assert plain.status[i] == 0 and not np.array_equal(borders(plain, i), borders(res, i)), i   # the test can tell them apart


def test_narrow_window_around_a_move_tables_guide(ctx):
    """a stride-5 move table needs five samples per base: the stalled reads at ~9 samples per k-mer"""
    reads = ctx["fam"]["stall_mv"]
    al = ctx["aligner"](gc.STALL_BAND)
    guides = []
    for r in reads:
        mv, ts = gc.moves_over_starts(r.starts, len(r.signal), stride=5)
        guides.append(G.guide_from_moves(mv, len(r.signal), len(r.sequence), gc.K, ts=ts))
    res = al.align_batch_guided(*sig_seq(reads), guides, gc.STALL_HALF_WIDTH)
    by_starts = al.align_batch_guided(*sig_seq(reads), [gc.true_guide(r) for r in reads], gc.STALL_HALF_WIDTH)
    for i, r in enumerate(reads):
        assert_is_the_model(res, i, model_of(ctx, al, r, guides[i], gc.STALL_HALF_WIDTH), "moves")
        assert by_starts.status[i] == 0 and np.array_equal(borders(res, i), borders(by_starts, i)), i


# ---- d ---------------------------------------------------------------------------------------------------------------------
def test_infeasible_guides_cost_their_reads_only(ctx, guided_a):
    reads = ctx["fam"]["a"]
    big = [i for i, r in enumerate(reads) if r.n_kmers + 1 >= 140][:2]      # room for a jump of 2 hw + 4 columns
    idx = sorted(big + [i for i in range(len(reads)) if i not in big][:6])
    assert len(big) == 2 and len(idx) == 8
    hw = 25
    guides = {i: gc.diagonal(reads[i]) for i in idx}
    cut, jump = big
    Ncol = reads[cut].n_kmers + 1
    guides[cut] = np.minimum(guides[cut], Ncol - 1 - (hw + 1)).astype(np.int32)      # the last window ends at column N - 2
    g = guides[jump].copy()
    s = len(g) // 4
    g[s:] = np.maximum(g[s:], g[s - 1] + 2 * hw + 4)                                  # consecutive windows are disjoint
    assert g.max() <= reads[jump].n_kmers and g[s] - g[s - 1] == 2 * hw + 4
    guides[jump] = g.astype(np.int32)
    sub = [reads[i] for i in idx]
    res = ctx["aligner"](50).align_batch_guided(*sig_seq(sub), [guides[i] for i in idx], hw)
    for k, i in enumerate(idx):
        if i in (cut, jump):
            assert res.status[k] == 5 and res.error(k) == Z_MISMATCH and res.n_segments[k] == 0, (i, res.status[k])
        else:
            assert res.status[k] == 0 and same_bits(res.Z[k], guided_a.Z[i]) and np.array_equal(borders(res, k), borders(guided_a, i)), i
            assert np.array_equal(probs(res, k), probs(guided_a, i)), i


# ---- e ---------------------------------------------------------------------------------------------------------------------
def test_more_reads_than_workgroups(ctx):
    reads = ctx["fam"]["e"]
    assert len(reads) == 600 and all(20 <= r.n_kmers <= 60 for r in reads) and len({len(r.signal) for r in reads}) > 200
    al = ctx["aligner"](16)
    al.set_mem_budget(48 << 20)   # arenas for a few dozen workgroups at the most: every one of them is reused many times
    try:
        res = al.align_batch_guided(*sig_seq(reads), [gc.diagonal(r) for r in reads], 8)   # B = 19: the 64-thread shape
    finally:
        al.set_mem_budget(0)
    assert_is_the_oracle(res, ctx["refs"]("e", 16), "e")


# ---- f ---------------------------------------------------------------------------------------------------------------------
def test_riders_equal_the_unguided_call(ctx, guided_a):
    reads = ctx["fam"]["a"]
    al = ctx["aligner"](50)
    guides = [gc.diagonal(r) for r in reads]
    al.set_event_stats(True)
    al.set_segment_scores(8)
    al.set_kmer_summary(True)
    try:
        al.reset_kmer_summary()
        plain = al.align_batch(*sig_seq(reads))
        ks_plain = al.kmer_summary()
        al.reset_kmer_summary()
        guided = al.align_batch_guided(*sig_seq(reads), guides, 25)
        ks_guided = al.kmer_summary()
    finally:
        al.set_event_stats(False)
        al.set_segment_scores(0)
        al.set_kmer_summary(False)
    assert np.array_equal(plain.signal_positions, guided.signal_positions) and np.array_equal(plain.status, guided.status)
    for col in ("level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity"):
        x, y = getattr(plain, col), getattr(guided, col)
        assert x is not None and y is not None and np.array_equal(x.view(np.uint64), y.view(np.uint64)), col
    assert ks_plain["totals"] == ks_guided["totals"] and ks_plain["totals"]["reads_ok"] == len(reads)
    for x, y in zip(ks_plain["limbs"], ks_guided["limbs"]):
        assert np.array_equal(x, y)
    assert np.array_equal(guided.signal_positions[:guided_a.signal_positions.size], guided_a.signal_positions)


def test_guided_band_margins_are_the_restatement(ctx):
    a, st = ctx["fam"]["a"], ctx["fam"]["stall"]
    al = ctx["aligner"](50)
    al.set_band_margin(True)
    try:
        ga = al.align_batch_guided(*sig_seq(a), [gc.diagonal(r) for r in a], 25)
        hw = gc.STALL_HALF_WIDTH
        guides = [gc.true_guide(r) for r in st]
        # one read's guide shifted by exactly the half width: the path runs along the window's lower edge (slack 0)
        guides[0] = np.minimum(guides[0].astype(np.int64) + hw, st[0].n_kmers).astype(np.int32)
        gs = al.align_batch_guided(*sig_seq(st), guides, hw)
    finally:
        al.set_band_margin(False)

    def check(res, reads, gds, half, what):
        seen_zero = 0
        for i, r in enumerate(reads):
            assert res.status[i] == 0, (what, i, res.error(i))
            want = gc.guided_margin(borders(res, i) + 1, len(r.signal) + 1, r.n_kmers + 1, gds[i], half)
            got = (int(res.band_margin_low[i]), int(res.band_margin_high[i]), int(res.band_edge_rows[i]))
            assert got == want, (what, i, got, want)
            seen_zero += min(want[0], want[1]) == 0
        return seen_zero

    check(ga, a, [gc.diagonal(r) for r in a], 25, "a")
    assert check(gs, st, guides, hw, "stall") >= 1
    assert int(gs.band_margin_low[0]) == 0 and int(gs.band_edge_rows[0]) > 30


# ---- g ---------------------------------------------------------------------------------------------------------------------
def test_refusals_budget_and_cells(ctx):
    reads = ctx["fam"]["b"][:4]
    al = ctx["aligner"](50)
    guides = [gc.diagonal(r) for r in reads]
    flat = np.concatenate(guides)
    with al.batch(*sig_seq(reads)) as b:
        b.set_guide(flat, 12)
        with pytest.raises(ValueError, match="dyn_batch_train: the batch carries a guide"):
            b.train()
        for setter, arg, text in ((al.set_rescale, 2, "dyn_aligner_set_rescale"), (al.set_border_confidence, 4, "dyn_aligner_set_border_confidence")):
            setter(arg)
            try:
                with pytest.raises(ValueError, match="dyn_batch_align: the batch carries a guide .* does not combine with " + text):
                    b.align(True)
            finally:
                setter(0)
        b.align(True)
        res = b.fetch()
        assert (res.status == 0).all()
        assert b.timing()["cells"] == sum((len(r.signal) + 1) * (2 * 12 + 1) for r in reads)
        assert b.arena_bytes() == len(reads) * ((25 * max(len(r.signal) + 1 for r in reads) * (2 * 12 + 3) + 255) // 256 * 256)
        with pytest.raises(ValueError, match="dyn_batch_set_guide: the batch has already run"):
            b.set_guide(flat, 12)
    # a budget that holds the short reads' lattices and not the long one's: that read alone is too large
    long_read, short = ctx["fam"]["a"][int(np.argmax([len(r.signal) for r in ctx["fam"]["a"]]))], reads
    need_long = 25 * (len(long_read.signal) + 1) * (2 * 25 + 3)
    need_short = max(25 * (len(r.signal) + 1) * (2 * 25 + 3) for r in short)
    assert need_short * 2 < need_long
    al.set_mem_budget(need_long - 4096)
    try:
        mix = short[:2] + [long_read] + short[2:]
        res = al.align_batch_guided(*sig_seq(mix), [gc.diagonal(r) for r in mix], 25)
    finally:
        al.set_mem_budget(0)
    assert res.status.tolist() == [0, 0, 8, 0, 0] and res.error(2) == "Read too large for the device memory budget"


# ---- h: the two windows of the banded-lattice kernel against each other -----------------------------------------------------------
WIDE_BAND = 600


@pytest.fixture(scope="module")
def wide(models):
    """ONE unguided batch at band 600 whose launch holds three different B = 2 bw + 3: two reads of 620-700 k-mers (bw = 300, one
    of them behind pad + 20-60 A's: a structural tie at its start) and one read each with N = 501 and N = 560 lattice columns
    (bw = N / 2 = 250 and 280). Its align, Z-only, asynchronous and train results, computed once."""
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6101, 1, "rna004", mean, sd, (628, 708))
    reads += synth.make_reads(6102, 1, "rna004", mean, sd, (628, 708), polya=(20, 60))
    reads += synth.make_reads(6103, 1, "rna004", mean, sd, 508) + synth.make_reads(6104, 1, "rna004", mean, sd, 567)
    N = [len(r.sequence) - 9 + 2 for r in reads]
    bw = [min(WIDE_BAND // 2, n // 2) for n in N]
    assert all(621 <= n <= 701 for n in N[:2]) and N[2:] == [501, 560] and bw == [300, 300, 250, 280]
    assert reads[1].sequence[:29] == "A" * 29
    al = Aligner(models["syn9"], "rna004", band=WIDE_BAND)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    w = dict(al=al, reads=reads, sig=sig, seq=seq, N=N, bw=bw, guides=[G.diagonal_guide(len(r.signal), n) for r, n in zip(reads, N)])
    w["align"] = al.align_batch(sig, seq, True)
    w["zonly"] = al.align_batch(sig, seq, False)
    with al.align_async(*synth.pack_reads(reads), True) as t:
        w["async"] = t.wait()
    w["train"] = al.train_batch(sig, seq)
    yield w
    al.close()


def u64(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def test_the_diagonal_window_is_a_diagonal_guide_bit_for_bit(wide):
    """Every read of the unguided batch again, alone, through the guide window: a diagonal guide at half_width = the read's own
    bw. What separates the two window policies is all here: per-read against per-launch half width, the N / 2 clamp with odd N,
    the fixed against the computed seed column, an LDS row stride larger than a read's B."""
    al = wide["al"]
    for i, r in enumerate(wide["reads"]):
        g = al.align_batch_guided([r.signal], [r.sequence], [wide["guides"][i]], wide["bw"][i])
        gz = al.align_batch_guided([r.signal], [r.sequence], [wide["guides"][i]], wide["bw"][i], calc_probabilities=False)
        assert g.status[0] == 0 and gz.status[0] == 0, (i, g.error(0), gz.error(0))
        want = g.read(0)
        for what in ("align", "async"):
            res = wide[what]
            assert res.status[i] == 0, (what, i, res.error(i))
            got = res.read(i)
            assert np.array_equal(got["signal_positions"], want["signal_positions"]), (what, i)
            assert np.array_equal(got["sequence_positions"], want["sequence_positions"]), (what, i)
            assert len(got["signal_positions"]) == wide["N"][i] - 1
            assert np.array_equal(u64(got["Z"]), u64(want["Z"])), (what, i, got["Z"], want["Z"])
            assert np.array_equal(u64(got["probabilities"]), u64(want["probabilities"])), (what, i)
        z = wide["zonly"]
        assert z.status[i] == 0 and z.n_segments[i] == 0 and gz.n_segments[0] == 0
        assert np.array_equal(u64(z.Z[i]), u64(gz.Z[0])) and np.array_equal(u64(z.Z[i]), u64(want["Z"])), i


def test_diagonal_window_train_against_a_diagonal_guide(wide):
    """train_batch against train_batch_guided(diagonal guide, the read's bw). Z and both transition counts: the same bits. The
    emission sums are held to rtol 1e-7 / atol 1e-9 (the bar of test_any_band_long_reads_equal_the_oracle_bit_for_bit), NOT to
    array_equal, by design: under the diagonal window a thread keeps a column's running sum in a register and flushes it when
    the band moves, under the guide window every row adds into the column's word in memory -- the same terms in the same
    order, grouped differently, so the last bits differ."""
    al, tr = wide["al"], wide["train"]
    for i, r in enumerate(wide["reads"]):
        g = al.train_batch_guided([r.signal], [r.sequence], [wide["guides"][i]], wide["bw"][i])
        assert tr.status[i] == 0 and g.status[0] == 0, (i, tr.error(i), g.error(0))
        assert np.array_equal(u64(tr.Z[i]), u64(g.Z[0])), i
        assert np.array_equal(u64(tr.trans_counts[2 * i:2 * i + 2]), u64(g.trans_counts[:2])), i
        a0, cnt = int(tr.em_offsets[i]), int(tr.em_count[i])
        assert cnt > 100 and cnt == int(g.em_count[0]) and np.array_equal(tr.em_code[a0:a0 + cnt], g.em_code[:cnt]), i
        assert np.allclose(tr.em_weight[a0:a0 + cnt], g.em_weight[:cnt], rtol=1e-7, atol=1e-9), i
        assert np.allclose(tr.em_sum[a0:a0 + cnt], g.em_sum[:cnt], rtol=1e-7, atol=1e-9), i


def test_wide_reads_arena(wide):
    """dyn_batch_arena_bytes of the wide reads' batch: one arena per workgroup, min(reads, compute units) of them (the API does
    not report the compute units; an MI355X has 256, and no GPU this suite runs on has fewer than the four reads), each the
    largest read's lattice at 25 B per band slot for align, 16 B for train, nothing for the Z-only job"""
    al, reads = wide["al"], wide["reads"]
    max_T = max(len(r.signal) + 1 for r in reads)
    assert max(range(4), key=lambda i: (len(reads[i].signal) + 1) * (2 * wide["bw"][i] + 3)) < 2    # the largest lattice: a bw = 300 read
    assert max_T == max(len(r.signal) + 1 for r in reads[:2])
    groups = min(len(reads), 256)
    slots = max_T * (2 * 300 + 3)
    with al.batch(wide["sig"], wide["seq"]) as b:
        b.align(True)
        assert b.arena_bytes() == groups * ((25 * slots + 255) // 256 * 256)
        b.train()
        assert b.arena_bytes() == groups * ((16 * slots + 255) // 256 * 256)
        b.align(False)
        assert b.arena_bytes() == 0
        assert (b.fetch().status == 0).all()
