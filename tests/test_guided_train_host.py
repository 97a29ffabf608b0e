"""CPU: the host half of guided-band training (dyn_batch_train_guided, Aligner.train_batch_guided, dynamont-train --guide-moves).
The entry point's refusals on a handle without a device; the NumPy restatement of the guided training statistics
(tests/guided_train_cases.py) against the CPU oracle's train() -- on diagonal guides, where the window is the oracle's band,
and on covering guides against band 4093 --; the purpose, shown on the CPU first: on stalled reads the band around the fixed
diagonal puts between 7 % and 82 % of a read's posterior mass on other k-mers than the whole lattice does, and a window of
half width 16 around the true starts (or a move table's guide) does not; and the front end of ``--guide-moves``: the guide
of a DNA read and of a reversed, padded RNA read from the BAM's mv tag, and the reads without one counted."""
import os
import re

import numpy as np
import pytest

import guided_band_cases as gc
import guided_train_cases as gt
from conftest import ROOT
from dynamont_amd import Aligner, _native as N, bam_io, synth
from dynamont_amd import guide as G
from dynamont_amd.segmentation import train as train_cli
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("native_lib")

TODAYS_REFUSAL = "dyn_batch_train: the batch carries a guide .* training inside a guided band is not supported"


# ------------------------------------------------------------------------------------------------------ the entry point
def test_symbol_header_and_abi(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION 10\b", hdr)
    assert re.search(r"^int dyn_batch_train_guided\(dyn_batch\* b\);", hdr, re.M)
    assert "/* (added within ABI 10) dyn_batch_train inside the guide that dyn_batch_set_guide put on the batch */" in hdr
    assert N.SIGNATURES["dyn_batch_train_guided"][1] == [N.C.c_void_p] and getattr(native_lib, "dyn_batch_train_guided") is not None
    assert native_lib.dyn_batch_train_guided(None) == N.DYN_ERR_INVALID_ARGUMENT


def test_refusals_on_a_host_only_handle(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    reads = gc.build_reads(mean, sd)["b"][:3]
    al = Aligner(models["syn5"], gc.PORE, band=50, device="host")
    flat = np.concatenate([gc.diagonal(r) for r in reads])
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        with pytest.raises(ValueError, match="dyn_batch_train_guided: the batch carries no guide"):
            b.train_guided()
        b.set_guide(flat, 8)
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            b.train_guided()
        with pytest.raises(ValueError, match=TODAYS_REFUSAL):
            b.train()
    with pytest.raises(ValueError, match="signals and guides differ"):
        al.train_batch_guided([reads[0].signal], [reads[0].sequence], [], 4)
    with pytest.raises(ValueError, match="guide 0 holds 3 entries"):
        al.train_batch_guided([reads[0].signal], [reads[0].sequence], [np.zeros(3, dtype=np.int32)], 4)
    al.close()


# ------------------------------------------------------------------------------------------- the restatement and the oracle
@pytest.fixture(scope="module")
def ctx(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    al = Aligner(models["syn5"], gc.PORE, device="host")
    assert al.info.log_e1 == 0.0
    c = dict(fam=gc.build_reads(mean, sd), m1=float(al.info.log_m1), e2=float(al.info.log_e2), model=models["syn5"],
             pore=synth.PORES[gc.PORE][0], oracles={})
    al.close()

    def oracle(band):
        if band not in c["oracles"]:
            c["oracles"][band] = Oracle(c["model"], c["pore"], band)
        return c["oracles"][band]

    c["oracle"] = oracle
    return c


def model_of(ctx, orc, r, guide, hw):
    """the model's transition logs come from the aligner's info (Oracle.train's log_m1 / log_e2 are the reference's transition
    EXPECTATIONS)"""
    km = orc.kmers(r.sequence)
    mean, sd = orc.table()
    return gt.model_train(r.signal, km, mean[km], sd[km], ctx["m1"], ctx["e2"], guide, hw)


def held_to_the_oracle(ctx, reads, guides, hws, band, what):
    orc = ctx["oracle"](band)
    worst = np.zeros(4)
    for i, r in enumerate(reads):
        mo = model_of(ctx, orc, r, guides[i], hws[i])
        ref = orc.train(r.signal, r.sequence, dense=False)
        assert mo.ok, (what, i)
        worst = np.maximum(worst, gt.check_against_oracle(mo.codes, mo.m1, mo.e2, ref, r.signal, (what, i)))
    print("%-28s %2d reads: weight %.3g  sum %.3g  sumsq %.3g  |sum w - S| / S %.3g" % ((what, len(reads)) + tuple(worst)))
    return worst


@pytest.mark.parametrize("name,band", [("a", 50), ("a2", 270)])
def test_restatement_equals_the_oracles_train_with_a_diagonal_guide(ctx, name, band):
    reads = ctx["fam"][name]
    hws = [min(band // 2, (r.n_kmers + 1) // 2) for r in reads]
    held_to_the_oracle(ctx, reads, [gc.diagonal(r) for r in reads], hws, band, "%s diagonal, band %d" % (name, band))
    if name == "a":      # on a diagonal guide the model's Z is the oracle's to Z_RTOL (its bits on this family)
        orc = ctx["oracle"](band)
        for r, hw in list(zip(reads, hws))[:4]:
            mo = model_of(ctx, orc, r, gc.diagonal(r), hw)
            ref = orc.train(r.signal, r.sequence, dense=False)
            assert abs(mo.Z - ref["Z"]) <= gc.Z_RTOL * abs(ref["Z"])


def test_restatement_equals_the_oracle_at_the_widest_band_under_random_staircases(ctx):
    """the window of tests/test_gpu_guided_band.py's (b): as wide as the longest read has columns, so every guide covers"""
    reads = ctx["fam"]["b"]
    hw = max(r.n_kmers + 1 for r in reads)
    rng = np.random.default_rng(11)
    guides = [gc.random_staircase(rng, len(r.signal), r.n_kmers + 1) for r in reads]
    assert max(int(np.diff(g).max()) for g in guides) >= 6
    held_to_the_oracle(ctx, reads, guides, [hw] * len(reads), 4093, "b random staircase")


def test_the_purpose_on_the_cpu(ctx):
    """every stalled read, none left out: the narrow guided window gives band 4093's statistics, band 50 does not"""
    stall, stall_mv = ctx["fam"]["stall"], ctx["fam"]["stall_mv"]
    assert len(stall) == 16 and len(stall_mv) == 6
    hw = gc.STALL_HALF_WIDTH
    held_to_the_oracle(ctx, stall, [gc.true_guide(r) for r in stall], [hw] * 16, 4093, "stall, true starts")
    guides = []
    for r in stall_mv:
        mv, ts = gc.moves_over_starts(r.starts, len(r.signal), stride=5)
        guides.append(G.guide_from_moves(mv, len(r.signal), len(r.sequence), gc.K, ts=ts))
    held_to_the_oracle(ctx, stall_mv, guides, [hw] * 6, 4093, "stall_mv, move table")
    shifts = []
    for r in stall:
        w50 = ctx["oracle"](gc.STALL_BAND).train(r.signal, r.sequence, dense=False)["weight"]
        w_all = ctx["oracle"](4093).train(r.signal, r.sequence, dense=False)["weight"]
        shifts.append(gt.weight_shift(w50, w_all, len(r.signal)))
    print("stall: sum |w_50 - w_4093| / S between %.3f and %.3f" % (min(shifts), max(shifts)))
    assert min(shifts) > 0.05, shifts


# ---------------------------------------------------------------------------------------------------- dynamont-train's front
def test_parse_default_is_off():
    base = ["-r", "x", "-b", "y", "-o", "z", "-p", "rna002"]
    assert train_cli.parse(base).guide_moves == 0
    assert train_cli.parse(base + ["--guide-moves", "16"]).guide_moves == 16


def _with_moves(tmp_path, pore, seed, moves_of):
    """a small dataset of three reads (the project's own writers); the BAM is rewritten with an mv tag per read:
    moves_of(i, n_bases) -> int8 table or None"""
    k = synth.PORES[pore][2]
    mean, sd = synth.model_values(k, seed=7, stdev=0.25)
    reads = synth.make_reads(seed, 3, pore, mean, sd, (40, 60))
    data = str(tmp_path / pore)
    os.makedirs(data)
    _, bam, expected = synth.write_dataset(data, "gm", reads, pore, seed=seed, basecalls="bam")
    recs = []
    for i, rec in enumerate(bam_io.iter_bam(bam)):
        tags = {t: rec.get_tag(t) for t in ("qs", "ns", "ts", "fn", "sm", "sd")}
        mv = moves_of(i, len(rec.query_sequence))
        if mv is not None:
            tags["mv"] = mv
        recs.append((rec.query_name, rec.query_sequence, tags))
    out = os.path.join(data, "gm_mv.bam")
    bam_io.write_bam(out, recs)
    return data, out, expected, k


def every_other_block(n_bases, stride=5):
    """base b moves in block 2 b: it starts at sample 2 * stride * b"""
    flags = np.zeros(2 * n_bases, dtype=np.int8)
    flags[0::2] = 1
    return np.concatenate([[stride], flags]).astype(np.int8)


def test_read_items_builds_the_guide_of_a_dna_read_and_counts_reads_without_moves(tmp_path):
    def moves_of(i, n_bases):
        return [every_other_block(n_bases), None, np.array([5, 0, 0, 0], dtype=np.int8)][i]   # a table, no tag, no move

    data, bam, expected, k = _with_moves(tmp_path, "dna_r9", 31, moves_of)
    for raw in (False, True):
        items = list(train_cli.read_items(data, bam, "dna_r9", 0.0, raw=raw, guide_moves=16, k=k))
        assert items[1:] == ["noguide", "noguide"] and len(items[0]) == 4
        sig, seq, _, g = items[0]
        S = len(sig[0]) if raw else len(sig)
        assert seq == expected[0][1] and S == len(expected[0][0])
        # k-mer j (column j + 1) starts with its centre base j + 2, at sample 10 (j + 2): centre(s) = #{j: 10 (j + 2) <= s}
        n_cols = len(seq) - k + 2
        want = np.clip(np.arange(S) // 10 - 1, 0, n_cols - 1)
        assert g.dtype == np.int32 and g.tolist() == want.tolist()
    # off: the items of the parent, three entries each, whatever the tags
    items = list(train_cli.read_items(data, bam, "dna_r9", 0.0, raw=False))
    assert len(items) == 3 and all(len(x) == 3 for x in items)


def test_read_items_builds_the_guide_of_an_rna_read_after_reversal_and_pad(tmp_path):
    data, bam, expected, k = _with_moves(tmp_path, "rna002", 32, lambda i, n_bases: every_other_block(n_bases))
    items = list(train_cli.read_items(data, bam, "rna002", 0.0, raw=False, guide_moves=16, k=k))
    assert len(items) == 3
    recs = list(bam_io.iter_bam(bam))
    padded = 0
    for (sig, seq, _, g), rec, exp in zip(items, recs, expected):
        assert seq == exp[1] and seq.startswith("A" * 9)
        S, n_cols = len(sig), len(seq) - k + 2
        pad = len(seq) - len(rec.query_sequence)                   # 9 where the basecall had lost its polyA, else 0
        padded += pad == 9
        # the table counts bases in signal order = the reversed basecall: aligner base b >= pad is move b - pad, at sample
        # 10 (b - pad); the pad's bases take the first move's start, sample 0. k-mer j starts with base j + 2.
        starts = 10 * np.maximum(np.arange(n_cols - 1) + k // 2 - pad, 0)
        want = np.clip(np.searchsorted(starts, np.arange(S), side="right"), 0, n_cols - 1)
        assert g.tolist() == want.tolist()
    assert padded >= 1
