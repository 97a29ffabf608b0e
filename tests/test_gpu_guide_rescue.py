"""GPU (-m gpu): the guide rescue (dyn_aligner_set_guide_rescue, Aligner.set_guide_rescue) -- the plain alignment of every read,
then a self-guided second alignment of ONLY the reads whose diagonal band margin flags them, inside the same batch or ticket
(guide_rescue.hip; k_auto_guide and the refining k_band_reads behind a device-side list). Expectations come from the CPU
(tests/guide_rescue_cases.py, recomputed by tests/test_guide_rescue_host.py); the yardsticks on the device are the same
handle's plain ``align_batch`` and ``align_batch_auto``, and "equal" means bit for bit.
  1. a mixed batch: 24 of family a and the 16 stall reads interleaved, a NaN read and two reads that fail validation
  2. the same reads as tickets: float64, raw, four in flight; plain tickets around a rescue ticket on a handle with sessions
  3. the three kernel shapes (64 x 1, 64 x 4, 256 x 16)
  4. the empty and the full list
  5. half width 2: reads of 2, 3, 4, 6 and 8 alignments behind the list, one of them not converged
  6. the riders: event stats, segment scores, band margins, k-mer summary
  7. (code 2 is covered on the CPU: tests/test_guide_rescue_host.py::test_arena_formula_and_t_fit says why)
  8. the two kernels on buffers of the test's own: the selection against its Python restatement over several chunks, and a
     merge with one rescue that failed (code 3: the plain bits stay), one that ended ok and one read that was not listed
Yardsticks are computed once per module and left unchanged. No torch in this process."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import auto_guide_cases as ac
import guide_rescue_cases as rc
import guided_band_cases as gc
from conftest import ROOT
from types import SimpleNamespace
from dynamont_amd import Aligner, _native, synth
from oracle.pyoracle import Oracle

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

HW, REFINE = 16, 8
ROW_COLS = ("signal_positions", "sequence_positions", "probabilities", "states")


def sig_seq(reads):
    return [r.signal for r in reads], [r.sequence for r in reads]


def packed(reads):
    return synth.pack_reads([synth.SynthRead(r.signal, r.sequence) for r in reads])


def assert_same_reads(x, y, ix, iy, cols=ROW_COLS):
    """reads ix of x carry the bytes of reads iy of y: status, Z, rows"""
    for i, j in zip(ix, iy):
        assert x.status[i] == y.status[j] and x.n_segments[i] == y.n_segments[j], (i, j)
        assert np.float64(x.Z[i]).tobytes() == np.float64(y.Z[j]).tobytes(), (i, j)
        a, b, m = int(x.seg_offsets[i]), int(y.seg_offsets[j]), int(x.n_segments[i])
        for col in cols:
            assert getattr(x, col)[a:a + m].tobytes() == getattr(y, col)[b:b + m].tobytes(), (col, i, j)


def rescued(al, reads, m, hw=HW, refine=REFINE):
    al.set_guide_rescue(m, hw, refine)
    try:
        return al.align_batch(*sig_seq(reads), True)
    finally:
        al.set_guide_rescue(0, 0)


def check(res, plain, auto, flagged, auto_of):
    """res: the rescue's result over some reads; plain: the plain result over the same reads; auto: align_batch_auto over the
    flagged ones, auto_of[i] = where read i sits in it. Codes, then every read against its yardstick."""
    n = res.n
    want_code = np.zeros(n, dtype=np.uint8)
    want_code[list(flagged)] = 1
    assert res.rescue is not None and res.rescue.dtype == np.uint8 and res.rescue.tolist() == want_code.tolist()
    rest = [i for i in range(n) if i not in set(flagged)]
    assert_same_reads(res, plain, rest, rest)
    for i in rest:
        assert res.error(i) == plain.error(i)
        assert res.guide_rounds[i] == 0 and res.guide_converged[i] == 0
    assert_same_reads(res, auto, flagged, [auto_of[i] for i in flagged])
    assert [int(res.guide_rounds[i]) for i in flagged] == [int(auto.guide_rounds[auto_of[i]]) for i in flagged]
    assert [int(res.guide_converged[i]) for i in flagged] == [int(auto.guide_converged[auto_of[i]]) for i in flagged]
    for i in flagged[:1]:
        assert res.read(i)["rescue"] == 1


@pytest.fixture(scope="module")
def ctx(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    al = Aligner(models["syn5"], gc.PORE, band=rc.BAND)
    fam = gc.build_reads(mean, sd)
    reads, stall_at, a_at = rc.mixed(fam)
    edge = ac.edge_reads(*synth.code_order_table(mean, sd, gc.K, False))
    bad_char = SimpleNamespace(signal=fam["b"][0].signal, sequence=fam["b"][0].sequence[:20] + "X" + fam["b"][0].sequence[21:])
    too_short = SimpleNamespace(signal=fam["b"][1].signal[:5], sequence=fam["b"][1].sequence)
    # 40 reads, then a read whose plain alignment fails on the device (NaN) and two that fail validation, in the middle and last
    batch = reads[:20] + [bad_char] + reads[20:] + [edge["nan"], too_short]
    at = lambda i: i if i < 20 else i + 1  # noqa: E731
    c = dict(al=al, fam=fam, model=models["syn5"], batch=batch, stall_at=[at(i) for i in stall_at], a_at=[at(i) for i in a_at],
             failed=[20, 41, 42])
    c["flagged"] = [c["stall_at"][i] for i in rc.STALL_FLAGGED_M1]
    c["plain"] = al.align_batch(*sig_seq(batch), True)
    c["auto"] = al.align_batch_auto(*sig_seq(fam["stall"]), HW, REFINE)
    c["auto_of"] = {p: i for i, p in enumerate(c["stall_at"])}
    yield c
    al.close()


# ---- 1. the mixed batch -----------------------------------------------------------------------------------------------------------
def test_mixed_batch(ctx):
    plain, auto = ctx["plain"], ctx["auto"]
    assert plain.rescue is None and [int(plain.status[i] != 0) for i in ctx["failed"]] == [1, 1, 1]
    assert (np.delete(plain.status, ctx["failed"]) == 0).all()
    res = rescued(ctx["al"], ctx["batch"], 1)
    check(res, plain, auto, ctx["flagged"], ctx["auto_of"])
    # the rescued reads carry the borders of the oracle at band 4093, which their plain rows do not
    full = Oracle(ctx["model"], synth.PORES[gc.PORE][0], 4093)
    for i in ctx["flagged"]:
        r = ctx["batch"][i]
        want = full.align(r.signal, r.sequence, True)["signal_positions"]
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        assert np.array_equal(res.signal_positions[a:a + m], want), i
        assert not np.array_equal(plain.signal_positions[a:a + m], want), i
    assert [int(res.guide_rounds[i]) for i in ctx["flagged"]] == [rc.CHAIN_HW16_ROUNDS] * 12
    assert [int(res.guide_converged[i]) for i in ctx["flagged"]] == [1] * 12
    with pytest.raises(RuntimeError):
        res.read(ctx["failed"][0])
    assert res.read(ctx["a_at"][0])["rescue"] == 0
    # the switch is sampled per job: off again, the same handle gives the plain result and no codes
    again = ctx["al"].align_batch(*sig_seq(ctx["batch"]), True)
    assert again.rescue is None and again.guide_rounds is None
    assert_same_reads(again, plain, range(plain.n), range(plain.n))
    # the Z-only job ignores the switch
    ctx["al"].set_guide_rescue(1, HW, REFINE)
    try:
        z = ctx["al"].align_batch(*sig_seq(ctx["batch"]), False)
    finally:
        ctx["al"].set_guide_rescue(0, 0)
    assert z.rescue is None and np.array_equal(z.status == 0, plain.status == 0)


def test_refine_one_is_the_prepass_and_one_alignment(ctx):
    stall = ctx["fam"]["stall"]
    want = ctx["al"].align_batch_auto(*sig_seq(stall), HW, 1)
    res = rescued(ctx["al"], stall, rc.M_ALL, HW, 1)
    assert res.rescue.tolist() == [1] * 16
    assert_same_reads(res, want, range(16), range(16))
    assert res.guide_rounds.tolist() == want.guide_rounds.tolist() == [1] * 16 and res.guide_converged.tolist() == [0] * 16


# ---- 2. tickets -------------------------------------------------------------------------------------------------------------------
def ticket(al, reads, m, hw=HW, refine=REFINE):
    al.set_guide_rescue(m, hw, refine)
    try:
        return al.align_async(*packed(reads), True)
    finally:
        al.set_guide_rescue(0, 0)


def test_ticket_and_four_in_flight(ctx):
    al = ctx["al"]
    tickets = [ticket(al, ctx["batch"], 1) for _ in range(4)]
    try:
        for t in tickets:
            res = t.wait()
            check(res, ctx["plain"], ctx["auto"], ctx["flagged"], ctx["auto_of"])
            assert t.timing()["launches"] == 1
    finally:
        for t in tickets:
            t.close()
    # a result object refilled by a plain ticket carries no codes
    with al.align_async(*packed(ctx["batch"]), True, out=res) as t:
        r2 = t.wait()
        assert r2.rescue is None and r2.guide_rounds is None
        assert_same_reads(r2, ctx["plain"], range(r2.n), range(r2.n))


def test_raw_ticket(ctx):
    al = ctx["al"]
    reads = [ctx["batch"][i] for i in sorted(ctx["stall_at"] + ctx["a_at"][:8])]
    rng = np.random.default_rng(8201)
    shift, scale = rng.uniform(400, 500, len(reads)), rng.uniform(60, 90, len(reads))
    raw = [np.round(r.signal * sc + sh).astype(np.int16) for r, sh, sc in zip(reads, shift, scale)]
    seq = [r.sequence for r in reads]
    with al.batch_raw(raw, seq, shift, scale) as b:
        b.align(True)
        plain = b.fetch()
        sig = b.signals()
    off = np.zeros(len(raw) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(v) for v in raw])
    seq_off = np.zeros(len(seq) + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seq])
    al.set_band_margin(True)
    al.set_guide_rescue(1, HW, REFINE)
    try:
        t = al.align_raw_async(np.concatenate(raw), off, shift, scale, "".join(seq).encode(), seq_off)
    finally:
        al.set_guide_rescue(0, 0)
        al.set_band_margin(False)
    with t:
        res = t.wait()
    flagged = np.flatnonzero(res.rescue == 1).tolist()
    assert len(flagged) >= 6 and set(res.rescue.tolist()) <= {0, 1}        # (the int16 rounding moves the signal: the set is the device's)
    rest = [i for i in range(res.n) if i not in flagged]
    assert_same_reads(res, plain, rest, rest)
    # the flagged reads: align_batch_auto on the preprocessed samples the device holds
    pre = [sig[int(off[i]):int(off[i + 1])] for i in flagged]
    auto = al.align_batch_auto(pre, [seq[i] for i in flagged], HW, REFINE, guides=True)
    assert_same_reads(res, auto, flagged, range(len(flagged)))
    assert [int(res.guide_rounds[i]) for i in flagged] == auto.guide_rounds.tolist()
    # every read the plain margins flag at M = 1 is in the set, and no other
    al.set_band_margin(True)
    try:
        with al.batch_raw(raw, seq, shift, scale) as b:
            b.align(True)
            pm = b.fetch()
    finally:
        al.set_band_margin(False)
    assert flagged == [i for i in range(res.n) if min(int(pm.band_margin_low[i]), int(pm.band_margin_high[i])) < 1]
    for k, i in enumerate(flagged):                                        # margins of a rescued read: against its guided window
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        want = gc.guided_margin(res.signal_positions[a:a + m].astype(np.int64) + 1, len(pre[k]) + 1, m + 1, auto.guides[k], HW)
        assert (int(res.band_margin_low[i]), int(res.band_margin_high[i]), int(res.band_edge_rows[i])) == want, i
    for i in rest:
        assert (res.band_margin_low[i], res.band_margin_high[i], res.band_edge_rows[i]) == \
            (pm.band_margin_low[i], pm.band_margin_high[i], pm.band_edge_rows[i]), i


def test_plain_tickets_around_a_rescue_ticket_with_sessions(ctx, models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(7700 + j, 600, "rna004", mean, sd, (60, 120)) for j in range(2)]
    al = Aligner(models["syn9"], "rna004", band=rc.BAND, device=0)
    try:
        base = [al.align_batch(*sig_seq(d), True) for d in data]
        sub = data[0][:48]
        al.set_guide_rescue(1000, HW, REFINE)                              # a margin every read that met a real edge is below
        want = al.align_batch(*sig_seq(sub), True)
        al.set_guide_rescue(0, 0)
        assert (want.rescue == 1).sum() >= 24 and set(want.rescue.tolist()) <= {0, 1}
        tickets = [al.align_async(*packed(data[0]), True), ticket(al, sub, 1000), al.align_async(*packed(data[1]), True)]
        try:
            for t, b in ((tickets[0], base[0]), (tickets[2], base[1])):
                res = t.wait()
                assert res.rescue is None
                assert_same_reads(res, b, range(b.n), range(b.n))
            res = tickets[1].wait()
            assert res.rescue.tolist() == want.rescue.tolist() and tickets[1].timing()["launches"] == 1
            assert_same_reads(res, want, range(want.n), range(want.n))
            assert res.guide_rounds.tolist() == want.guide_rounds.tolist()
        finally:
            for t in tickets:
                t.close()
        st = al.session_stats()
        assert st["sessions"] >= 1 and st["aborted"] == 0
    finally:
        al.close()


# ---- 3. the three shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [16, 40, 130])
def test_every_shape_behind_the_list(ctx, hw):
    stall, some_a = ctx["fam"]["stall"], ctx["fam"]["a"][:8]
    reads = some_a[:4] + stall + some_a[4:]
    al = ctx["al"]
    plain = al.align_batch(*sig_seq(reads), True)
    auto = ctx["auto"] if hw == HW else al.align_batch_auto(*sig_seq(stall), hw, REFINE)
    res = rescued(al, reads, rc.M_ALL, hw)
    flagged = list(range(4, 20))
    check(res, plain, auto, flagged, {i: i - 4 for i in flagged})
    assert min(auto.guide_rounds) >= 2 and (auto.status == 0).all()


# ---- 4. the empty and the full list ---------------------------------------------------------------------------------------------------
def test_empty_list(ctx):
    reads = ctx["fam"]["a"]
    plain = ctx["al"].align_batch(*sig_seq(reads), True)
    res = rescued(ctx["al"], reads, 1)
    assert res.rescue.tolist() == [0] * 24 and not res.guide_rounds.any() and not res.guide_converged.any()
    assert_same_reads(res, plain, range(24), range(24))
    res = rescued(ctx["al"], reads, rc.M_ALL)                                 # M = 12 flags none of a either
    assert res.rescue.tolist() == [0] * 24
    assert_same_reads(res, plain, range(24), range(24))
    res = rescued(ctx["al"], ctx["fam"]["stall"], 0)                          # min_margin 0 flags nothing
    assert res.rescue.tolist() == [0] * 16


def test_full_list(ctx):
    res = rescued(ctx["al"], ctx["fam"]["stall"], rc.M_ALL)
    assert res.rescue.tolist() == [1] * 16
    assert_same_reads(res, ctx["auto"], range(16), range(16))
    assert res.guide_rounds.tolist() == ctx["auto"].guide_rounds.tolist() == [rc.CHAIN_HW16_ROUNDS] * 16
    assert res.guide_converged.tolist() == [1] * 16


# ---- 5. several rounds behind the list ------------------------------------------------------------------------------------------------
def test_half_width_two_takes_up_to_eight_alignments(ctx):
    stall = ctx["fam"]["stall"]
    al = ctx["al"]
    auto = al.align_batch_auto(*sig_seq(stall), 2, REFINE)
    res = rescued(al, ctx["batch"], 1, 2, REFINE)
    check(res, ctx["plain"], auto, ctx["flagged"], ctx["auto_of"])
    assert tuple(int(res.guide_rounds[i]) for i in ctx["flagged"]) == rc.CHAIN_HW2_ROUNDS
    still_open = tuple(s for s, i in zip(rc.STALL_FLAGGED_M1, ctx["flagged"]) if res.guide_converged[i] == 0)
    assert still_open == rc.CHAIN_HW2_OPEN
    assert (res.status[ctx["flagged"]] == 0).all()


# ---- 6. riders --------------------------------------------------------------------------------------------------------------------------
def test_riders_run_once_behind_the_rescue(ctx):
    al = ctx["al"]
    stall, a_reads = ctx["fam"]["stall"], ctx["fam"]["a"][:8]
    reads = a_reads[:4] + stall + a_reads[4:]
    flagged = [4 + i for i in rc.STALL_FLAGGED_M1]
    rest = [i for i in range(len(reads)) if i not in flagged]
    al.set_event_stats(True)
    al.set_segment_scores(8)
    al.set_band_margin(True)
    al.set_kmer_summary(True)
    try:
        al.reset_kmer_summary()
        plain = al.align_batch(*sig_seq([reads[i] for i in rest]), True)
        ks_plain = al.kmer_summary()
        al.reset_kmer_summary()
        auto = al.align_batch_auto(*sig_seq([reads[i] for i in flagged]), HW, REFINE, guides=True)
        ks_auto = al.kmer_summary()
        al.reset_kmer_summary()
        res = rescued(al, reads, 1)
        ks = al.kmer_summary()
    finally:
        al.set_event_stats(False)
        al.set_segment_scores(0)
        al.set_band_margin(False)
        al.set_kmer_summary(False)
        al.reset_kmer_summary()
    assert np.flatnonzero(res.rescue).tolist() == flagged
    cols = ROW_COLS + ("level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity")
    assert_same_reads(res, plain, rest, range(len(rest)), cols)
    assert_same_reads(res, auto, flagged, range(len(flagged)), cols)
    for col in ("band_margin_low", "band_margin_high", "band_edge_rows"):
        assert [int(getattr(res, col)[i]) for i in rest] == getattr(plain, col).tolist(), col          # against the diagonal
        assert [int(getattr(res, col)[i]) for i in flagged] == getattr(auto, col).tolist(), col        # against the guided window
    for k, i in enumerate(flagged):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        want = gc.guided_margin(res.signal_positions[a:a + m].astype(np.int64) + 1, len(reads[i].signal) + 1, m + 1, auto.guides[k], HW)
        assert (int(res.band_margin_low[i]), int(res.band_margin_high[i]), int(res.band_edge_rows[i])) == want, i
    # every read is summed once: the exact integers are plain(the others) + auto(the flagged)
    assert ks["totals"]["reads_ok"] == len(reads)
    for key, v in ks["totals"].items():
        assert v == ks_plain["totals"][key] + ks_auto["totals"][key], key
    for key in ("n_segments", "n_samples", "Q1", "Q2"):
        assert (ks[key] == ks_plain[key] + ks_auto[key]).all(), key


# ---- 8. the kernels on buffers of the test's own ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("guiderescue") / "libguiderescue.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/guide_rescue.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.gr_select_run.restype = C.c_int
    lib.gr_merge_run.restype = C.c_int
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("n_desc", [0, 1, 255, 256, 257, 1500])
def test_select_kernel_equals_the_restatement(harness, n_desc):
    rng = np.random.default_rng(9000 + n_desc)
    n = max(1, n_desc) + 7                                                 # reads no descriptor names stay 0
    NONE = rc.NONE
    status = rng.choice([0, 0, 0, 3, 7], size=n).astype(np.int32)
    low = rng.choice([0, 1, 11, 12, 100, NONE], size=n).astype(np.uint32)
    high = rng.choice([0, 1, 11, 12, 100, NONE], size=n).astype(np.uint32)
    read = rng.permutation(n)[:n_desc].astype(np.uint32)
    N_col = rng.choice([1, 2, 50], size=n_desc).astype(np.uint32)
    T = rng.integers(2, 5000, size=n_desc).astype(np.uint32)
    for min_margin, max_T in ((1, 5000), (12, 2500), (0, 5000), (12, 0)):
        want_code, want_list = rc.select(T, N_col, read, status, low, high, min_margin, max_T)
        code = np.full(n, 9, dtype=np.uint8)
        lst = np.zeros(max(1, n_desc), dtype=np.uint32)
        n_list = np.zeros(1, dtype=np.uint32)
        rcode = harness.gr_select_run(C.c_int(n_desc), p(T), p(N_col), p(read), C.c_int(n), p(status), p(low), p(high),
                                      C.c_uint32(min_margin), C.c_uint32(max_T), p(code), p(lst), p(n_list))
        assert rcode == 0
        assert int(n_list[0]) == len(want_list) and lst[:len(want_list)].tolist() == want_list, (n_desc, min_margin, max_T)
        assert (lst[len(want_list):n_desc] == NONE).all()                  # nothing written behind the list
        assert code.tolist() == want_code.tolist()


def test_merge_kernel_keeps_the_plain_answer_of_a_failed_rescue(harness):
    """three reads in descriptor order 2, 0, 1: read 0's rescue failed (code 3, the plain bits stay), read 1's ended ok (its state,
    segment rows and path rows from its first border on replace the plain ones), read 2 was not listed (untouched, code 0)"""
    T = np.array([300, 40, 700], dtype=np.uint32)                          # per descriptor: reads 2, 0, 1
    N_col = np.array([20, 9, 30], dtype=np.uint32)
    read = np.array([2, 0, 1], dtype=np.uint32)
    path_off = np.array([0, 300, 340], dtype=np.uint64)
    seg_off = np.array([37, 0, 8], dtype=np.uint64)                        # read 0: 8 rows, read 1: 29, read 2: 19
    n_rows, n_seg = 1040 + 5, 56 + 3
    rng = np.random.default_rng(9100)
    mk = lambda: (rng.random(n_rows), rng.integers(0, 1 << 31, n_rows).astype(np.uint32), rng.integers(1, 30, n_seg).astype(np.uint32))  # noqa: E731
    pp_in, pn_in, sr_in = mk()
    pp, pn, sr = mk()
    sr_in[8] = 123                                                         # read 1's first border of the rescue: lattice row 123
    status_in = np.array([3, 0, 0], dtype=np.int32)
    z_in = np.array([-1.5, -2.5, -3.5])
    status, z, nseg = np.zeros(3, dtype=np.int32), np.array([-10.0, -20.0, -30.0]), np.array([8, 29, 19], dtype=np.uint32)
    code = np.array([1, 1, 0], dtype=np.uint8)                             # what the selection left: provisional 1 where listed
    rounds, conv = np.array([5, 3, 0], dtype=np.uint32), np.array([0, 1, 0], dtype=np.uint32)
    lst = np.array([1, 2], dtype=np.uint32)                                # descriptors of reads 0 and 1
    before = [v.copy() for v in (pp, pn, sr, status, z, nseg)]
    rcode = harness.gr_merge_run(C.c_int(3), p(T), p(N_col), p(read), p(path_off), p(seg_off), C.c_int(2), p(lst), C.c_int(3),
                                 C.c_uint64(n_rows), C.c_uint64(n_seg), p(status_in), p(z_in), p(pp_in), p(pn_in), p(sr_in),
                                 p(status), p(z), p(nseg), p(pp), p(pn), p(sr), p(code), p(rounds), p(conv), C.c_int(0))
    assert rcode == 0
    assert code.tolist() == [3, 1, 0] and rounds.tolist() == [0, 3, 0] and conv.tolist() == [0, 1, 0]
    want_pp, want_pn, want_sr = before[0].copy(), before[1].copy(), before[2].copy()
    want_pp[340 + 123:340 + 700] = pp_in[340 + 123:340 + 700]
    want_pn[340 + 123:340 + 700] = pn_in[340 + 123:340 + 700]
    want_sr[8:37] = sr_in[8:37]
    assert pp.tobytes() == want_pp.tobytes() and pn.tobytes() == want_pn.tobytes() and sr.tobytes() == want_sr.tobytes()
    assert status.tolist() == [0, 0, 0] and z.tolist() == [-10.0, -2.5, -30.0] and nseg.tolist() == [8, 1, 19]
