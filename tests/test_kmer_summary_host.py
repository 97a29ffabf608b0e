"""CPU: the host half of the per-k-mer level summary. The derived columns of utils.kmer_summary_table against a
Python-int restatement of the definition on hand-made sums; the written TSV loads as a model through read_kmer_model and
through the library's own parser; the three new entry points exist and refuse a handle without a device / of mode ntk; the
device harness's inputs (tests/kmer_summary_cases.py) tell three deliberately wrong accumulations from the right one."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import kmer_summary_cases as ksc
from conftest import ROOT
from dynamont_amd import Aligner, _native as N, synth
from dynamont_amd._dynamont import int128_of_limbs, kmer_summary_from_limbs
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import (code_of_kmer, kmer_of_code, kmer_summary_table, merge_kmer_summaries,
                                             read_kmer_model, write_kmer_summary)

pytestmark = pytest.mark.usefixtures("native_lib")


def _summary(n_segments, n_samples, Q1, Q2):
    acc = {"n_segments": list(n_segments), "n_samples": list(n_samples), "Q1": list(Q1), "Q2": list(Q2),
           "totals": dict.fromkeys(ksc.TOTALS, 0)}
    cols, totals = ksc.limbs(acc)
    return kmer_summary_from_limbs(cols, totals)


def _nearest(fr):
    """the double nearest to an exact Fraction (int / int true division is correctly rounded)"""
    return fr.numerator / fr.denominator


# hand-made sums: (n_segments, n_samples, Q1, Q2). Q1 = m * n * 2^40, Q2 = (v + m^2) * n * 2^40 for mean m, variance v
HAND = [
    (3, 30, 30 * (1 << 40) * 5 // 4, 30 * (1 << 40) * (25 * 4 + 1 * 16) // 64),   # mean 1.25, variance 0.25
    (2, 7, -7 * (1 << 40) * 3, 7 * (1 << 40) * 10),                                # NEGATIVE Q1: mean -3, variance 1
    (1, 1, -(1 << 70) - 12345, (1 << 100) + (1 << 64) + 7),                        # beyond the 2^64 limb, both signs
    (5, 11, (1 << 64) - 1, (1 << 64)),                                             # the limb boundary itself
    (4, 9, (1 << 64), (1 << 65) - 1),
    (0, 0, 0, 0),                                                                  # never met: the model's values
    (6, 12, 12 * (1 << 40) * 2, 12 * (1 << 40) * 4),                               # zero variance: the model's values
    (1, 3, 3, 5),                                                                  # a few units of 2^-40
    (7, 1 << 54, (1 << 94) + 1, (1 << 96)),                                        # n_samples beyond 2^53
    (1, 2, -1, 1),
]


def test_table_against_the_python_int_restatement():
    n = len(HAND)
    rng = np.random.default_rng(3)
    mm, ms = rng.normal(0, 1, n), rng.uniform(0.1, 0.3, n)
    s = _summary(*zip(*HAND))
    assert [int(v) for v in s["Q1"]] == [h[2] for h in HAND] and [int(v) for v in s["Q2"]] == [h[3] for h in HAND]   # limbs round-trip
    t = kmer_summary_table(s, mm, ms)
    for c, (nseg, nsamp, Q1, Q2) in enumerate(HAND):
        if nseg == 0:
            assert (t["level_mean"][c], t["level_stdv"][c], t["dwell_mean"][c], bool(t["fitted"][c])) == (mm[c], ms[c], 0.0, False)
            continue
        # the definition, step by step: every step is the double nearest to the exact result of its operands
        m1 = _nearest(Fraction(Q1)) * 2.0 ** -40
        mean = _nearest(Fraction(m1) / Fraction(float(nsamp)))
        ex2 = _nearest(Fraction(_nearest(Fraction(Q2)) * 2.0 ** -40) / Fraction(float(nsamp)))
        var = _nearest(Fraction(ex2) - Fraction(_nearest(Fraction(mean) * Fraction(mean))))
        sd = math.sqrt(max(0.0, var))
        assert t["dwell_mean"][c] == _nearest(Fraction(float(nsamp)) / Fraction(float(nseg))), c
        if sd == 0.0:
            assert (t["level_mean"][c], t["level_stdv"][c], bool(t["fitted"][c])) == (mm[c], ms[c], False), c
        else:
            assert (t["level_mean"][c], t["level_stdv"][c], bool(t["fitted"][c])) == (mean, sd, True), c
    assert t["level_mean"][0] == 1.25 and t["level_stdv"][0] == 0.5 and t["dwell_mean"][0] == 10.0
    assert t["level_mean"][1] == -3.0 and t["level_stdv"][1] == 1.0
    assert not t["fitted"][6] and t["fitted"][2] and t["level_mean"][2] < -2.0 ** 29
    assert np.array_equal(t["model_mean"], mm) and np.array_equal(t["model_stdv"], ms)


def test_rint_ties_and_limbs_of_the_restatement():
    h = 2.0 ** -41
    assert [ksc.rint_scaled(v * h) for v in (1, 3, 5, -1, -3, -5, 1.5, -1.5)] == [0, 2, 2, 0, -2, -2, 1, -1]
    assert [ksc.rint_scaled(v * h, truncate=True) for v in (1, 3, 5, -1, -3, -5, 1.5, -1.5)] == [0, 1, 2, 0, -1, -2, 0, 0]
    assert ksc.segment_q(np.array([2.0 ** 30])) == (1, 1 << 70, 1 << 100)
    assert ksc.segment_q(np.array([2.0 ** 32])) is None and ksc.segment_q(np.array([np.nan])) is None
    assert ksc.segment_q(np.array([np.nextafter(2.0 ** 32, 0.0)]))[2] == (1 << 104) - (1 << 52)
    assert ksc.segment_q(np.array([-0.0, 5e-324])) == (2, 0, 0)
    lo = np.array([0, 1, ksc.M64, 0], dtype=np.uint64)
    hi = np.array([0, 0, ksc.M64, 1 << 63], dtype=np.uint64)
    assert int128_of_limbs(lo, hi).tolist() == [0, 1, -1, -(1 << 127)]
    a = _summary([1, 2], [3, 4], [-5, 1 << 70], [6, 7])
    b = _summary([1, 0], [1, 0], [-(1 << 70), -(1 << 70)], [1 << 100, 0])
    m = merge_kmer_summaries([a, b])
    assert m["n_segments"].tolist() == [2, 2] and m["n_samples"].tolist() == [4, 4]
    assert m["Q1"].tolist() == [-5 - (1 << 70), 0] and m["Q2"].tolist() == [6 + (1 << 100), 7]


@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna002", 5)])
def test_written_file_loads_as_a_model(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    mm, ms = al.model_table()
    n = al.num_kmers
    rng = np.random.default_rng(9)
    nseg = rng.integers(0, 4, n)
    nsamp = nseg * rng.integers(1, 30, n)
    q1 = [int(s * rng.normal(0, 1) * (1 << 40)) for s in nsamp]
    q2 = [int(s * (abs(rng.normal(0, 1)) + (a / max(s, 1) / (1 << 40)) ** 2) * (1 << 40)) for s, a in zip(nsamp, q1)]
    nseg[5], nsamp[5], q1[5], q2[5] = 2, 8, 8 << 40, 8 << 40   # zero variance
    s = _summary(nseg.tolist(), nsamp.tolist(), q1, q2)
    out = str(tmp_path / "summary.tsv")
    t = write_kmer_summary(out, s, model, mm, ms, al.rna)
    assert t["fitted"].sum() > n // 2 and (~t["fitted"]).sum() > n // 8 and not t["fitted"][5]
    lines = open(out).read().split("\n")
    assert lines[0] == "kmer\tlevel_mean\tlevel_stdv\tn_segments\tn_samples\tdwell_mean\tmodel_mean\tmodel_stdv" and lines[-1] == ""
    names = synth.read_model_file(model)[0]
    assert [ln.split("\t")[0] for ln in lines[1:-1]] == names                       # the model file's own order
    for name, ln in zip(names, lines[1:-1]):
        c = code_of_kmer(name, al.rna)
        assert kmer_of_code(c, k, al.rna) == name
        p = ln.split("\t")
        assert (float(p[1]), float(p[2]), int(p[3]), int(p[4]), float(p[5]), float(p[6]), float(p[7])) == (
            t["level_mean"][c], t["level_stdv"][c], nseg[c], nsamp[c], t["dwell_mean"][c], mm[c], ms[c])
        assert p[1] == repr(float(t["level_mean"][c])) and p[7] == repr(float(ms[c]))
    km = read_kmer_model(out)                                                        # the Python loader
    assert all(km[name] == (t["level_mean"][code_of_kmer(name, al.rna)], t["level_stdv"][code_of_kmer(name, al.rna)]) for name in names)
    al2 = Aligner(out, pore, device="host")                                          # the library's parser
    m2, s2 = al2.model_table()
    assert np.array_equal(m2.view(np.uint64), t["level_mean"].view(np.uint64))
    assert np.array_equal(s2.view(np.uint64), t["level_stdv"].view(np.uint64))
    al.close()
    al2.close()


def test_the_new_symbols(native_lib, models):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    abi = int(re.search(r"#define DYN_ABI_VERSION (\d+)\b", hdr).group(1))
    assert abi >= 10                                                 # (the entry points are additive; the number is pinned elsewhere)
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_kmer_summary", "dyn_aligner_kmer_summary_fetch", "dyn_aligner_kmer_summary_reset"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    al = Aligner(models["syn9"], "rna004", device="host")
    info = N.DynInfo()
    assert native_lib.dyn_aligner_info(al._h, C.byref(info)) == 0 and info.abi_version == abi
    al.close()


def test_entry_points_refuse_what_they_cannot_serve(native_lib, models):
    assert native_lib.dyn_aligner_set_kmer_summary(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_kmer_summary_reset(None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")          # no device: as every entry point that needs one
    for on in (True, False):
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            al.set_kmer_summary(on)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.kmer_summary()
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.reset_kmer_summary()
    al.close()
    ntk = Aligner(models["syn9"], "rna004", mode="resquiggle", device="host")
    with pytest.raises(ValueError, match="modes ntk / resquiggle"):
        ntk.set_kmer_summary(True)
    ntk.close()


def test_cli_flag():
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).kmer_summary == ""
    assert seg.parse(base + ["--kmer-summary", "out.tsv"]).kmer_summary == "out.tsv"


def test_kernels_compile_with_the_products_flags_without_scratch(tmp_path):
    """tests/device_math/kmer_summary.hip builds with the product's flags; the compiler's resource remarks show 256-thread
    kernels without scratch and within 8 KB of static LDS -- they run beside a resident workgroup."""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "kmer_summary.hip"), "-o", str(tmp_path / "libks.so")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(scratch) == 2 and scratch == [0, 0] and max(lds) <= 8192, (scratch, lds)


@pytest.fixture(scope="module")
def batch():
    return ksc.build_batch()


def test_harness_batch_holds_the_cases(batch):
    b = batch
    lens = [len(x) for _, segs in b.reads for _, x in segs]
    assert set(lens) >= {1, 63, 64, 65, 256, 257, 16384, 16385, 20001}
    assert (b.read != np.arange(len(b.read))).sum() > len(b.read) // 2                 # processing order is not read order
    failed = np.flatnonzero(b.status != 0)
    assert len(failed) == 1 and 0 < failed[0] < len(b.status) - 1
    ref = ksc.reference(b)
    assert ref["n_segments"][11] == 5000 and sum(len(segs) > 256 for _, segs in b.reads) >= 10   # many blocks on one k-mer
    assert ref["Q1"][12] == -(1 << 71) and ref["Q1"][13] > (1 << 70) and ref["Q2"][13] > (1 << 100)
    assert ref["Q2"][14] == (1 << 104) - (1 << 52) and ref["n_segments"][14] == 1      # 2^64 itself (twice) skipped, its neighbour kept
    assert ref["totals"]["skipped_segments"] == 4 and ref["n_segments"][15] == 1
    assert ref["n_segments"][16] == 3 and ref["n_samples"][16] == 75 and ref["Q1"][16] == 0 and ref["Q2"][16] == 0
    assert ref["Q1"][17] == 4 and ref["Q1"][18] == -4 and ref["Q1"][19] == 1 and ref["Q1"][20] == -1
    assert ref["Q2"][22] == 3 * 4095 * 4095 * (1 << 40) > (1 << 65)
    assert ref["totals"]["reads_ok"] == len(b.reads) - 1
    assert ref["totals"]["segments"] == sum(ref["n_segments"]) and ref["totals"]["samples"] == sum(ref["n_samples"])
    # a sub-range of reads (a merged launch whose members did not all ask) is a different, smaller sum
    part = ksc.reference(b, 2, 9)
    assert 0 < part["totals"]["segments"] < ref["totals"]["segments"] and part["totals"]["reads_ok"] == 6


@pytest.mark.parametrize("how", ["carry_dropped", "truncated", "no_sign_extension"])
def test_inputs_tell_a_wrong_accumulation_apart(batch, how):
    right = ksc.limbs(ksc.reference(batch))[0]
    wrong = ksc.wrong_limbs(batch, how)
    differs = [name for name, r, w in zip(("n_segments", "n_samples", "q1_lo", "q1_hi", "q2_lo", "q2_hi"), right, wrong)
               if not np.array_equal(r, w)]
    assert differs, how
    assert set(differs) <= {"q1_lo", "q1_hi", "q2_lo", "q2_hi"}
    if how == "carry_dropped":
        assert "q1_hi" in differs and "q2_hi" in differs
    if how == "no_sign_extension":
        assert differs == ["q1_hi"]
    # the same accumulation done right, limb by limb in read order, is the reference (the wrong ones differ by their fault alone)
    assert all(np.array_equal(r, w) for r, w in zip(right, ksc.wrong_limbs(batch, "none")))
