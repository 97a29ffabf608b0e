"""CPU: the host half of the guide rescue (dyn_aligner_set_guide_rescue, Aligner.set_guide_rescue): self-guide only the reads
whose band margin flags them.
  1. the fixture, recomputed: which reads of families a, b and stall the diagonal margins (CPU oracle at band 50,
     ``band_margin_cases.brute``) flag at M = 1, 12 and 18 -- the values tests/guide_rescue_cases.py pins for the GPU tests
  2. the selection rule: the g++ build of the product's ``rescue_decide`` (guide_rescue_kernels.hpp) against a Python
     restatement on every input class, the arena formula and T_fit
  3. the NumPy chain (pre-pass, then refinement over ``guided_band_cases.model_align``) at half widths 16 and 2
  4. every new refusal and argument range with its text, on a handle without a device
(What a job under the switch computes needs a device: tests/test_gpu_guide_rescue.py.)"""
import os
import re

import numpy as np
import pytest

import auto_guide_cases as ac
import band_margin_cases as bm
import guide_rescue_cases as rc
import guided_band_cases as gc
from conftest import ROOT
from dynamont_amd import Aligner, _native as N, synth
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("native_lib")


@pytest.fixture(scope="module")
def ctx(models, tmp_path_factory):
    _, mean, sd = synth.read_model_file(models["syn5"])
    al = Aligner(models["syn5"], gc.PORE, device="host")
    c = dict(fam=gc.build_reads(mean, sd), m1=float(al.info.log_m1), e2=float(al.info.log_e2), model=models["syn5"],
             narrow=Oracle(models["syn5"], synth.PORES[gc.PORE][0], rc.BAND), full=Oracle(models["syn5"], synth.PORES[gc.PORE][0], 4093),
             host=ac.build_host(tmp_path_factory.mktemp("ag_host")), rule=rc.build_host(tmp_path_factory.mktemp("gr_host")))
    al.close()
    return c


@pytest.fixture(scope="module")
def plain(ctx):
    """family -> per read (min margin, borders at band 50 == borders at band 4093)"""
    out = {}
    for name in ("a", "b", "stall"):
        out[name] = []
        for r in ctx["fam"][name]:
            res = ctx["narrow"].align(r.signal, r.sequence, True)
            T, Ncol = len(r.signal) + 1, r.n_kmers + 1
            low, high, _ = bm.brute(res["signal_positions"].astype(np.int64) + 1, T, Ncol, min(rc.BAND // 2, Ncol // 2), float(Ncol) / float(T))
            want = ctx["full"].align(r.signal, r.sequence, True)
            out[name].append((min(low, high), np.array_equal(res["signal_positions"], want["signal_positions"])))
    return out


# ---- 1. the fixture ------------------------------------------------------------------------------------------------------------
def test_the_flagged_sets(ctx, plain):
    fam = ctx["fam"]
    assert (len(fam["a"]), len(fam["b"]), len(fam["stall"])) == (24, 16, 16)
    assert (min(len(r.signal) + 1 for r in fam["a"]), max(len(r.signal) + 1 for r in fam["a"])) == (657, 3644)
    assert (min(len(r.signal) + 1 for r in fam["stall"]), max(len(r.signal) + 1 for r in fam["stall"])) == (308, 507)
    assert (min(r.n_kmers + 1 for r in fam["stall"]), max(r.n_kmers + 1 for r in fam["stall"])) == (80, 148)
    a, b, stall = ([m for m, _ in plain[k]] for k in ("a", "b", "stall"))
    print("minimum margins: a %s, b %s, stall %s" % (sorted(a), sorted(b), stall))
    assert min(a) >= rc.A_MIN_MARGIN and all(same for _, same in plain["a"])
    assert min(b) >= rc.B_MIN_MARGIN
    assert not any(same for _, same in plain["stall"])                     # all 16 differ from band 4093
    flagged = tuple(i for i, m in enumerate(stall) if m < 1)
    assert flagged == rc.STALL_FLAGGED_M1 and len(flagged) == 12
    assert {i: m for i, m in enumerate(stall) if m >= 1} == rc.STALL_UNFLAGGED_M1
    assert all(m < rc.M_ALL for m in stall) and min(a + b) >= rc.M_ALL     # M = 12: all of stall, none of a or b
    assert rc.M_ALL <= rc.B_MIN_MARGIN <= rc.A_MIN_MARGIN


def test_mixed_order_interleaves_the_two_families(ctx):
    reads, stall_at, a_at = rc.mixed(ctx["fam"])
    assert len(reads) == 40 and len(stall_at) == 16 and len(a_at) == 24 and sorted(stall_at + a_at) == list(range(40))
    assert [reads[i] is r for i, r in zip(stall_at, ctx["fam"]["stall"])] == [True] * 16
    assert stall_at[0] > 0 and stall_at[-1] < 39 and max(np.diff(stall_at)) >= 2   # neither a prefix nor a suffix nor one block


# ---- 2. the rule -----------------------------------------------------------------------------------------------------------------
def test_rule_host_build_equals_the_restatement_on_every_input_class(ctx):
    rng = np.random.default_rng(20261019)
    NONE = rc.NONE
    margins = [0, 1, 2, 11, 12, 13, 1000, NONE - 1, NONE]
    n = 600
    status = rng.choice([0, 0, 0, 1, 3, 7], size=n).astype(np.int32)       # failed reads among them
    low = rng.choice(margins, size=n).astype(np.uint32)
    high = rng.choice(margins, size=n).astype(np.uint32)
    read = rng.permutation(n).astype(np.uint32)                            # descriptors in another order than the reads
    N_col = rng.choice([1, 2, 3, 50], size=n).astype(np.uint32)            # N = 1: no border at all
    T = rng.integers(2, 5000, size=n).astype(np.uint32)
    seen = set()
    for min_margin in (0, 1, 12, 13, NONE):
        for max_T in (0, 2500, 5000):
            want_code, want_list = rc.select(T, N_col, read, status, low, high, min_margin, max_T)
            code, lst = rc.host_select(ctx["rule"], T, N_col, read, status, low, high, min_margin, max_T)
            assert code.tolist() == want_code.tolist() and lst == want_list, (min_margin, max_T)
            assert lst == sorted(lst)                                      # descriptor order
            if min_margin == 0:
                assert not code.any() and lst == []                        # min_margin 0 flags nothing
            if max_T == 0:
                assert lst == [] and set(code.tolist()) <= {0, 2}
            seen |= set(code.tolist())
            for k in range(n):
                r = int(read[k])
                if status[r] != 0 or N_col[k] < 2 or (low[r] == NONE and high[r] == NONE):
                    assert code[r] == 0, (k, r)
                elif code[r]:
                    assert (code[r] == 2) == (T[k] > max_T)
    assert seen == {0, 1, 2}
    # single decisions, spelled out
    d = rc.decide
    assert d(0, 50, 100, NONE, NONE, NONE, 1000) == 0                     # never a real edge: +infinity, below no threshold
    assert d(0, 50, 100, NONE, 0, 1, 1000) == 1 and d(0, 50, 100, 0, NONE, 1, 1000) == 1
    assert d(0, 50, 100, 1, 5, 1, 1000) == 0 and d(0, 50, 100, 1, 5, 2, 1000) == 1
    assert d(3, 50, 100, 0, 0, 1, 1000) == 0 and d(0, 1, 100, 0, 0, 1, 1000) == 0
    assert d(0, 50, 1000, 0, 0, 1, 1000) == 1 and d(0, 50, 1001, 0, 0, 1, 1000) == 2


def test_arena_formula_and_t_fit(ctx):
    """T_fit / max_T_rescuable on the CPU: the longest T whose arena fits the room. (The GPU suite does not separate reads by a
    memory budget: at test shapes a budget below one guided arena -- 0.3 to 3 MB -- leaves the plain stage's page pool two pages.)"""
    assert rc.band_arena_bytes(507, 16) == (507 * 35 * 25 + 255) // 256 * 256 == 443648
    assert rc.band_arena_bytes(3644, 16) == 3188736
    Ts = [len(r.signal) + 1 for r in ctx["fam"]["stall"]] + [len(r.signal) + 1 for r in ctx["fam"]["a"]]
    assert rc.t_fit(Ts, 16, 443648) == 507 and rc.t_fit(Ts, 16, 443647) < 507
    assert rc.t_fit(Ts, 16, 10 ** 9) == max(Ts) == 3644 and rc.t_fit(Ts, 16, 1000) == 0
    # with room for the stall reads only, a flagged long read gets code 2 and the stall reads code 1
    fit = rc.t_fit(Ts, 16, 443648)
    assert rc.decide(0, 100, 507, 0, 0, 1, fit) == 1 and rc.decide(0, 100, 3644, 0, 0, 1, fit) == 2


# ---- 3. the chain ----------------------------------------------------------------------------------------------------------------
def params(ctx, r):
    km = ctx["full"].kmers(r.sequence)
    mean, sd = ctx["full"].table()
    return np.ascontiguousarray(mean[km]), np.ascontiguousarray(sd[km]), -np.log(np.ascontiguousarray(sd[km]))


def chain(ctx, r, hw, max_rounds):
    mean, sd, nls = params(ctx, r)
    g = ac.host_guide(ctx["host"], r.signal, mean, sd, nls, ctx["m1"], ctx["e2"], hw)
    return ac.refine(r.signal, mean, sd, ctx["m1"], ctx["e2"], g, hw, max_rounds)


def test_chain_at_half_width_16(ctx):
    for name, n in (("stall", 16), ("stall_mv", 6)):
        assert len(ctx["fam"][name]) == n
        for i, r in enumerate(ctx["fam"][name]):
            rounds, conv, _, mo, _ = chain(ctx, r, 16, 8)
            assert (rounds, conv, mo.ok) == (rc.CHAIN_HW16_ROUNDS, 1, True), (name, i)
            want = ctx["full"].align(r.signal, r.sequence, True)
            assert np.array_equal(mo.signal_positions, want["signal_positions"].astype(np.int64)), (name, i)


def test_chain_at_half_width_2_takes_several_rounds(ctx):
    got, still_open = [], []
    for i in rc.STALL_FLAGGED_M1:
        rounds, conv, _, mo, _ = chain(ctx, ctx["fam"]["stall"][i], 2, 8)
        assert mo.ok, i                                                    # all end ok
        got.append(rounds)
        if not conv:
            still_open.append(i)
    print("alignments per read at half width 2:", got)
    assert tuple(got) == rc.CHAIN_HW2_ROUNDS and tuple(still_open) == rc.CHAIN_HW2_OPEN


@pytest.mark.parametrize("hw", [1, 2, 4, 8, 16])
def test_no_rescue_fails_on_the_cpu_model(ctx, hw):
    """why code 3 is tested at kernel level: the pre-pass keeps the windows connected, so the chain ends ok at every half width"""
    for i, r in enumerate(ctx["fam"]["stall"]):
        assert chain(ctx, r, hw, 2)[3].ok, (hw, i)


# ---- 4. entry points, ranges, refusals ---------------------------------------------------------------------------------------------
def test_header_declares_the_entry_points_within_abi_10(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert "DYN_ABI_VERSION 10" in hdr
    assert re.search(r"int dyn_aligner_set_guide_rescue\(dyn_aligner\* a, int min_margin, uint32_t half_width, uint32_t max_rounds\);", hdr)
    assert re.search(r"int dyn_batch_fetch_rescue\(dyn_batch\* b, uint8_t\* code, uint32_t\* rounds, uint32_t\* converged, uint64_t n\);", hdr)
    for name in ("dyn_aligner_set_guide_rescue", "dyn_batch_fetch_rescue"):
        assert name in N.SIGNATURES and getattr(native_lib, name) is not None
    assert "guide_rescue.hip" in N.SOURCES and "guide_rescue_kernels.hpp" in N.HEADERS
    assert native_lib.dyn_aligner_set_guide_rescue(None, 1, 16, 8) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_batch_fetch_rescue(None, None, None, None, 0) == N.DYN_ERR_INVALID_ARGUMENT


def test_argument_ranges_and_off(models):
    al = Aligner(models["syn5"], gc.PORE, device="host")
    try:
        assert al._guide_rescue == (0, 0, 8)
        for bad in (2047, 100000):
            with pytest.raises(ValueError, match=r"dyn_aligner_set_guide_rescue: half_width %d is outside \[1, 2046\]" % bad):
                al.set_guide_rescue(1, bad)
        with pytest.raises(ValueError, match=r"dyn_aligner_set_guide_rescue: min_margin -1 is negative"):
            al.set_guide_rescue(-1, 16)
        for bad in (0, 65):
            with pytest.raises(ValueError, match=r"dyn_aligner_set_guide_rescue: max_rounds %d is outside \[1, 64\]" % bad):
                al.set_guide_rescue(1, 16, bad)
        assert al._guide_rescue == (0, 0, 8)                               # a refused call changes nothing
        for m, hw, rounds in ((0, 1, 1), (1, 2046, 64), (12, 16, 8)):
            al.set_guide_rescue(m, hw, rounds)
            assert al._guide_rescue == (m, hw, rounds)
        al.set_guide_rescue(-5, 0, 0)                                      # off: the other two are not looked at
        assert al._guide_rescue == (0, 0, 8)
    finally:
        al.close()
    ntk = Aligner(models["syn5"], gc.PORE, mode="resquiggle", device="host")
    try:
        with pytest.raises(ValueError, match="dyn_aligner_set_guide_rescue: modes ntk / resquiggle have no align"):
            ntk.set_guide_rescue(1, 16)
    finally:
        ntk.close()


def test_every_refusal_with_its_text(ctx):
    reads = ctx["fam"]["b"][:3]
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    pk = synth.pack_reads([synth.SynthRead(r.signal, r.sequence) for r in reads])
    al = Aligner(ctx["model"], gc.PORE, band=rc.BAND, device="host")
    try:
        al.set_guide_rescue(1, 16, 8)
        others = ((lambda on: al.set_rescale(2 if on else 0), r"dyn_aligner_set_rescale\(a, iters > 0\)"),
                  (lambda on: al.set_border_confidence(8 if on else 0), r"dyn_aligner_set_border_confidence\(a, window > 0\)"),
                  (lambda on: al.set_auto_guide(16 if on else 0), r"dyn_aligner_set_auto_guide\(a, half_width > 0\)"))
        with al.batch(sig, seq) as b:
            for switch, text in others:
                switch(True)
                with pytest.raises(ValueError, match="dyn_batch_align: dyn_aligner_set_guide_rescue is on, which does not combine with " + text):
                    b.align(True)
                with pytest.raises(ValueError, match="dyn_batch_align_async: dyn_aligner_set_guide_rescue is on, which does not combine with " + text):
                    al.align_async(*pk)
                with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
                    b.align(False)                                         # the Z-only job ignores the switch
                switch(False)
            with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
                b.align(True)                                              # nothing left to refuse
            with pytest.raises(ValueError, match="dyn_batch_fetch_rescue: the batch was not aligned with calc_probabilities = 1 under"):
                rc.fetch_rescue(N.lib(), b._h, al, b.n)
            b.set_guide(np.concatenate([gc.diagonal(r) for r in reads]), 8)
            with pytest.raises(ValueError, match=r"dyn_batch_align: dyn_aligner_set_guide_rescue is on and the batch carries a guide"):
                b.align(True)
            al.set_guide_rescue(0, 0)
            with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
                b.align(True)                                              # off: the guided batch is a guided batch again
        al.set_guide_rescue(1, 16)
        with pytest.raises(ValueError, match="set_band_retry with set_guide_rescue"):
            al.set_band_retry(1)
        al.set_band_retry(0)                                               # turning the retry off is always allowed
        al.set_guide_rescue(0, 0)
    finally:
        al.close()


def test_band_retry_first_refuses_the_rescue(models):
    al = Aligner(models["syn5"], gc.PORE, device="host")
    try:
        al._band_retry = (1, 4093, 2)                                      # (set_band_retry itself needs a device for its margins)
        with pytest.raises(ValueError, match="set_guide_rescue with set_band_retry"):
            al.set_guide_rescue(1, 16)
        al.set_guide_rescue(1, 0)                                          # off is always allowed
    finally:
        al.close()


def test_multi_aligner_has_no_such_switch():
    from dynamont_amd import MultiAligner
    assert not hasattr(MultiAligner, "set_guide_rescue")


# ---- 5. the command's parser ---------------------------------------------------------------------------------------------------------
BASE = ["-r", "raw", "-b", "calls.bam", "-o", "out", "--mode", "basic", "-p", "rna004"]


def test_parser_names_defaults_and_exclusions(capsys):
    from dynamont_amd.segmentation import segment as seg_cli
    args = seg_cli.parse(BASE)
    assert (args.guide_rescue, args.guide_rescue_margin, args.guide_rounds) == (0, 1, 8)
    args = seg_cli.parse(BASE + ["--guide-rescue", "16", "--guide-rescue-margin", "12", "--guide-rounds", "4", "--event-stats",
                                 "--segment-scores", "8", "--kmer-summary", "k.tsv", "--band-report", "b.tsv", "--host-preprocess"])
    assert (args.guide_rescue, args.guide_rescue_margin, args.guide_rounds) == (16, 12, 4)
    for other, name in ((["--guide-auto", "16"], "--guide-auto"), (["--rescale-iters", "2"], "--rescale-iters"),
                        (["--border-confidence", "8"], "--border-confidence")):
        with pytest.raises(SystemExit) as e:
            seg_cli.parse(BASE + ["--guide-rescue", "16"] + other)
        assert e.value.code == 2
        assert "--guide-rescue and %s are mutually exclusive" % name in capsys.readouterr().err
        assert seg_cli.parse(BASE + other).guide_rescue == 0               # without the flag the other switch is accepted
    with pytest.raises(ValueError, match="--guide-rescue is not combined with --guide-auto"):
        seg_cli.segment("raw", "calls.bam", 1, "out", "m", "rna004", "basic", guide_rescue=16, guide_auto=16)


def test_band_report_lines_take_one_band_per_read():
    from dynamont_amd.segmentation import segment as seg_cli
    one = seg_cli.band_report_lines(["a", "b"], [10, 20], [3, 4], 50, [1, 0xFFFFFFFF], [2, 3], [0, 1])
    per = seg_cli.band_report_lines(["a", "b"], [10, 20], [3, 4], np.array([50, 32]), [1, 0xFFFFFFFF], [2, 3], [0, 1])
    assert one == ["a\t10\t3\t50\t1\t2\t0", "b\t20\t4\t50\t\t3\t1"]
    assert per == [one[0], "b\t20\t4\t32\t\t3\t1"]
