"""CPU: the host half of the per-site level summary (dyn_aligner_set_site_summary). The header text and the symbols; what a handle
without a device refuses and what it still shows of the staging call (its count check, consumed whatever the outcome); the
Python layer's dict from limbs; the kernels' footprint as the compiler reports it; and the device harness's inputs
(tests/site_summary_cases.py), which tell five deliberately wrong accumulations from the right one."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native as N, synth
from dynamont_amd._dynamont import site_summary_from_limbs

pytestmark = pytest.mark.usefixtures("native_lib")

SYMBOLS = ("dyn_aligner_set_site_summary", "dyn_aligner_stage_site_ids", "dyn_aligner_site_summary_fetch", "dyn_aligner_site_summary_reset")


def test_header_text_and_symbols(native_lib, models):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION (\d+)\b", hdr).group(1) == "10"        # added within ABI 10
    assert re.search(r"#define DYN_SITE_NONE 0xFFFFFFFFu\b", hdr)
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    flat = " ".join(hdr.split())
    assert "int dyn_aligner_set_site_summary(dyn_aligner* a, uint64_t num_sites);" in flat
    assert "int dyn_aligner_stage_site_ids(dyn_aligner* a, const uint32_t* site_ids, uint64_t count);" in flat
    assert ("int dyn_aligner_site_summary_fetch(dyn_aligner* a, uint64_t lo, uint64_t hi, uint64_t* n_rows, uint64_t* n_samples, "
            "uint64_t* dwell_sq, uint64_t* m1_lo, uint64_t* m1_hi, uint64_t* m2_lo, uint64_t* m2_hi, uint64_t totals[5]);") in flat
    assert "int dyn_aligner_site_summary_reset(dyn_aligner* a);" in flat
    assert N.DYN_SITE_NONE == 0xFFFFFFFF == ssc.NONE
    al = Aligner(models["syn9"], "rna004", device="host")
    info = N.DynInfo()
    assert native_lib.dyn_aligner_info(al._h, C.byref(info)) == 0 and info.abi_version == 10
    al.close()


def test_entry_points_refuse_what_they_cannot_serve(native_lib, models):
    assert native_lib.dyn_aligner_set_site_summary(None, 5) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_stage_site_ids(None, None, 0) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_summary_reset(None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")          # no device: DYN_ERR_DEVICE, as every entry point that needs one
    assert native_lib.dyn_aligner_set_site_summary(al._h, 100) == N.DYN_ERR_DEVICE
    for n in (100, 0):
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            al.set_site_summary(n)
    with pytest.raises(ValueError, match="not below DYN_SITE_NONE"):
        al.set_site_summary(0xFFFFFFFF)
    with pytest.raises(ValueError, match="num_sites must be >= 0"):
        al.set_site_summary(-1)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_summary(0, 0)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.reset_site_summary()
    assert native_lib.dyn_aligner_stage_site_ids(al._h, None, 3) == N.DYN_ERR_INVALID_ARGUMENT      # ids missing
    al.close()
    ntk = Aligner(models["syn9"], "rna004", mode="resquiggle", device="host")
    with pytest.raises(ValueError, match="modes ntk / resquiggle"):
        ntk.set_site_summary(10)
    ntk.close()
    with pytest.raises(NotImplementedError, match="MultiAligner has no per-site summary"):
        MultiAligner.set_site_summary(None, 10)


def test_staging_count_check_and_consumption_through_dyn_batch_create(models):
    """on a handle without a device dyn_batch_create builds the read table alone -- enough to see the staging rule: the count must
    equal the batch's characters, and whatever was staged is gone after ONE batch-creating call, failed or not"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(11, 3, "rna004", mean, sd, (30, 50))
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    bases = sum(len(s) for s in seq)
    al = Aligner(models["syn9"], "rna004", device="host")
    al.batch(sig, seq).close()                                       # nothing staged: fine
    al.batch(sig, seq, site_ids=np.arange(bases, dtype=np.uint32)).close()
    for wrong in (bases - 1, bases + 1, 0):
        with pytest.raises(ValueError, match=r"staged %d ids, the batch's sequences hold %d characters" % (wrong, bases)):
            al.batch(sig, seq, site_ids=np.zeros(wrong, dtype=np.uint32))
        al.batch(sig, seq).close()                                   # the refused call consumed them: the next one has none
    # consumed by a call that fails for ANOTHER reason too (no offsets): the wrong count staged here is never seen again
    ids = np.zeros(bases + 7, dtype=np.uint32)
    assert al._L.dyn_aligner_stage_site_ids(al._h, ids.ctypes.data_as(N.c_u32_p), ids.size) == N.DYN_OK
    h = C.c_void_p()
    assert al._L.dyn_batch_create(al._h, 3, None, None, None, None, C.byref(h)) == N.DYN_ERR_INVALID_ARGUMENT
    al.batch(sig, seq).close()
    # staging twice: the second array replaces the first
    al._stage_site_ids(np.zeros(1, dtype=np.uint32))
    al.batch(sig, seq, site_ids=np.zeros(bases, dtype=np.uint32)).close()
    with pytest.raises(ValueError, match="one-dimensional"):
        al.batch(sig, seq, site_ids=np.zeros((2, 2), dtype=np.uint32))
    al.close()


def test_dict_from_limbs():
    acc = ssc.empty(4)
    acc["n_rows"], acc["n_samples"], acc["dwell_sq"] = [1, 2, 0, 5], [3, 9, 0, 1 << 40], [9, 41, 0, (1 << 64) + 5]
    acc["M1"], acc["M2"] = [-5, (1 << 70) + 1, 0, -(1 << 100)], [7, 1 << 100, 0, (1 << 64) - 1]
    acc["totals"] = dict(zip(ssc.TOTALS, (4, 8, 12, 1, 2)))
    s = site_summary_from_limbs(*ssc.limbs(acc))
    assert s["M1"].tolist() == acc["M1"] and s["M2"].tolist() == acc["M2"]
    assert s["n_rows"].tolist() == acc["n_rows"] and s["dwell_sq"].tolist() == [9, 41, 0, 5]      # mod 2^64
    assert s["totals"] == acc["totals"] and len(s["limbs"]) == 7 and all(c.dtype == np.uint64 for c in s["limbs"])


def test_band_retry_is_refused_like_the_kmer_summary(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    al._site_summary = 10                                            # (the setter itself needs a device)
    with pytest.raises(ValueError, match="set_band_retry with set_site_summary"):
        al.set_band_retry(2)
    al._site_summary = 0
    al._band_retry = (2, 4093, 2)
    with pytest.raises(ValueError, match="set_site_summary with set_band_retry"):
        al.set_site_summary(10)
    al.close()


def test_kernels_compile_with_the_products_flags_beside_a_resident_workgroup(tmp_path):
    """tests/device_math/site_summary.hip builds with the product's flags; the compiler's resource remarks show two 256-thread
    kernels without scratch, within 13 KB of static LDS and 152 VGPRs -- they run beside a resident workgroup"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "site_summary.hip"), "-o", str(tmp_path / "libss.so")]
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == 2 and any("k_ssum_short" in n for n in names) and any("k_ssum_long" in n for n in names)
    assert scratch == [0, 0] and max(lds) <= 13 * 1024 and max(vgprs) <= 152, (scratch, lds, vgprs)


def test_the_kmer_summary_still_includes_the_shared_helpers():
    """the chunked sum, the double -> i128 conversion and the 128-bit add live in ONE header both features include"""
    src = {f: open(os.path.join(N.CSRC, f)).read() for f in ("kmer_summary_kernels.hpp", "site_summary_kernels.hpp", "exact_sum_kernels.hpp")}
    for f in ("kmer_summary_kernels.hpp", "site_summary_kernels.hpp"):
        assert '#include "exact_sum_kernels.hpp"' in src[f]
        assert "xs_to_i128(" in src[f] and "xs_add128(" in src[f] and "atomicAdd(" in src[f]
        assert not re.search(r"void \w+_to_i128\(|void \w+_add128\(", src[f])        # used, not defined again
    assert "__global__" not in src["exact_sum_kernels.hpp"]
    assert "site_summary.hip" in N.SOURCES and "exact_sum_kernels.hpp" in N.HEADERS and "site_summary_kernels.hpp" in N.HEADERS


def test_the_table_host_unit_is_built():
    """the host half of every per-site call lives in a translation unit of its own"""
    assert "site_table.cpp" in N.SOURCES


@pytest.fixture(scope="module")
def batch():
    return ssc.build_batch()


def test_harness_batch_holds_the_cases(batch):
    b = batch
    lens = [len(x) for _, segs in b.reads for _, x in segs]
    assert set(lens) >= {1, 63, 64, 65, 256, 257, 16384, 16385 + 7}
    ids = [s for _, segs in b.reads for s, _ in segs]
    assert {ssc.NONE, b.num_sites - 1, b.num_sites} <= set(ids)
    long_ids = {s for _, segs in b.reads for s, x in segs if len(x) > 256}
    assert {ssc.NONE, b.num_sites - 1, b.num_sites} <= long_ids                        # ... in the long kernel as well
    assert (b.read != np.arange(len(b.read))).sum() > len(b.read) // 2                 # processing order is not read order
    failed = np.flatnonzero(b.status != 0)
    assert len(failed) == 1 and 0 < failed[0] < len(b.status) - 1
    ref = ssc.reference(b)
    assert ref["n_rows"][11] == 600 and ref["n_rows"][12] == 300 and sum(len(segs) > 256 for _, segs in b.reads) >= 3
    assert ref["M1"][11] > (1 << 64) and ref["M1"][12] < -(1 << 64) and ref["M2"][11] > (1 << 84)   # past the low limb, both signs
    assert ref["n_rows"][14] == 1 and ref["M2"][14] == (1 << 104) - (1 << 52)          # m * m = 2^64 (twice) skipped, its neighbour kept
    assert ref["n_rows"][15] == 1 and ref["M1"][15] == 1 << 39                         # NaN / inf rows skipped, 0.5 kept
    assert ref["n_rows"][16] == 3 and ref["n_samples"][16] == 75 and ref["dwell_sq"][16] == 1 + 16 + 4900 and ref["M1"][16] == 0
    assert ref["M1"][17] == 4 and ref["M1"][18] == -4 and ref["M1"][19] == 1 and ref["M1"][20] == -1
    t = ref["totals"]
    assert t["reads_ok"] == len(b.reads) - 1 and t["rows_without_site"] == 9 and t["rows_skipped"] == 8
    assert t["rows_added"] == sum(ref["n_rows"]) and t["samples_added"] == sum(ref["n_samples"])
    assert max(ref["n_rows"][21:31]) == 3 and min(ref["n_rows"][21:31]) >= 1           # overlapping reads
    part = ssc.reference(b, 2, 9)
    assert 0 < part["totals"]["rows_added"] < t["rows_added"] and part["totals"]["reads_ok"] == 6


def test_restatement_of_one_row():
    h = 2.0 ** -41
    assert [ssc.row_terms([v * h])[1] for v in (1, 3, 5, -1, -3, -5, 1.5, -1.5)] == [0, 2, 2, 0, -2, -2, 1, -1]
    assert [ssc.row_terms([v * h], truncate=True)[1] for v in (1, 3, 5, -1, -3, -5, 1.5, -1.5)] == [0, 1, 2, 0, -1, -2, 0, 0]
    assert ssc.row_terms([2.0 ** 30] * 3) == (3, 1 << 70, 1 << 100)
    assert ssc.row_terms([2.0 ** 32]) is None and ssc.row_terms([1.0, np.nan]) is None and ssc.row_terms([np.inf]) is None
    assert ssc.row_terms([1.0, 2.0, 4.0]) == (3, round(Fraction(7.0 / 3.0) * (1 << 40)), round(Fraction((7.0 / 3.0) * (7.0 / 3.0)) * (1 << 40)))
    # m is a DIVISION: S1 * (1 / L) rounds twice and differs in m's last bit for some sums -- which shows in m1 where an ulp of m
    # is a unit of 2^-40 or more, i.e. at levels of 2^12 and beyond
    x = np.random.default_rng(1).normal(2.0 ** 22, 300.0, (400, 3))
    assert sum(ssc.row_terms(r) != ssc.row_terms(r, reciprocal=True) for r in x) > 10


@pytest.mark.parametrize("how", ["carry_dropped", "no_sign_extension", "truncated", "reciprocal"])
def test_inputs_tell_a_wrong_accumulation_apart(batch, how):
    right = ssc.limbs(ssc.reference(batch))[0]
    wrong = ssc.wrong_limbs(batch, how)
    names = ("n_rows", "n_samples", "dwell_sq", "m1_lo", "m1_hi", "m2_lo", "m2_hi")
    differs = [name for name, r, w in zip(names, right, wrong) if not np.array_equal(r, w)]
    assert differs, how
    assert set(differs) <= {"m1_lo", "m1_hi", "m2_lo", "m2_hi"}
    if how == "carry_dropped":
        assert "m1_hi" in differs and "m2_hi" in differs
    if how == "no_sign_extension":
        assert differs == ["m1_hi"]
    if how in ("truncated", "reciprocal"):
        assert "m1_lo" in differs and "m2_lo" in differs
    # the same accumulation done right, limb by limb in read order, is the reference (the wrong ones differ by their fault alone)
    assert all(np.array_equal(r, w) for r, w in zip(right, ssc.wrong_limbs(batch, "none")))


def test_a_row_is_keyed_by_the_base_in_the_middle_of_its_kmer():
    """row j <- ids[j + k // 2] (the row's sequence_pos): keyed by ids[j] the same read lands on other sites"""
    rng = np.random.default_rng(2)
    k, n_rows = 9, 30
    ids = np.arange(100, 100 + n_rows + k - 1, dtype=np.uint32)
    ids[10:13] = ssc.NONE
    sig = rng.normal(0, 1, 300)
    starts = np.sort(rng.choice(np.arange(1, 300), n_rows - 1, replace=False))
    starts = np.concatenate([[0], starts])
    right = ssc.add_aligned_read(ssc.empty(200), ids, k, sig, starts)
    wrong = ssc.add_aligned_read(ssc.empty(200), ids, k, sig, starts, shift=0)
    assert ssc.row_ids(ids, n_rows, k)[:3] == [104, 105, 106] and ssc.row_ids(ids, n_rows, k, shift=0)[:3] == [100, 101, 102]
    assert right["n_rows"] != wrong["n_rows"] and right["M1"] != wrong["M1"]
    assert right["n_rows"][104] == 1 and right["n_rows"][100] == 0 and wrong["n_rows"][100] == 1
    assert right["totals"]["rows_without_site"] == 3 == wrong["totals"]["rows_without_site"]
    assert [i for i, v in enumerate(right["n_rows"]) if v == 0 and 104 <= i < 104 + n_rows] == [110, 111, 112]


# ---- dynamont-resquiggle --site-summary: the flag, its refusals, the TSV ---------------------------------------------------------
def test_cli_flag():
    from dynamont_amd.segmentation import segment as seg
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).site_summary == ""
    assert seg.parse(base + ["--site-summary", "sites.tsv"]).site_summary == "sites.tsv"


def test_cli_refuses_a_bam_without_references_and_more_than_one_rank(models, tmp_path, monkeypatch):
    """both before anything is started: no aligner, no process group, no output file"""
    from dynamont_amd import bam_io
    from dynamont_amd.segmentation import segment as seg
    tags = dict(qs=12.5, ns=5000, ts=10, fn="reads.pod5", sm=90.0, sd=15.0)
    ubam, mapped = str(tmp_path / "u.bam"), str(tmp_path / "m.bam")
    bam_io.write_bam(ubam, [("r0", "ACGTACGTACGT", dict(tags))])
    bam_io.write_bam(mapped, [("r0", "ACGTACGTACGT", dict(tags), (0, 0, 3, [12 << 4]))], references=[("chrA", 100)])
    assert bam_io.bam_references(mapped) == (["chrA"], [100])
    out = str(tmp_path / "out.csv.zst")
    args = (str(tmp_path), ubam, 1, out, models["syn9"], "rna004", "basic")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="has no reference sequences"):
        seg.segment(*args, site_summary=str(tmp_path / "s.tsv"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="--site-summary runs in one process"):
        seg.segment(str(tmp_path), mapped, 1, out, models["syn9"], "rna004", "basic", site_summary=str(tmp_path / "s.tsv"))
    monkeypatch.delenv("WORLD_SIZE")
    with pytest.raises(ValueError, match="mapped .bam read by the native reader"):
        seg.segment(str(tmp_path), mapped, 1, out, models["syn9"], "rna004", "basic", host_preprocess=True, site_summary=str(tmp_path / "s.tsv"))
    with pytest.raises(ValueError, match="mapped .bam read by the native reader"):
        seg.segment(str(tmp_path), str(tmp_path / "calls.sam"), 1, out, models["syn9"], "rna004", "basic", site_summary=str(tmp_path / "s.tsv"))
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "s.tsv")


def test_reads_that_get_no_ids(tmp_path):
    """unmapped, secondary, supplementary, reverse strand, the CG placeholder and a CIGAR that does not cover the read get
    DYN_SITE_NONE throughout and are counted; the forward reads get their sites, RNA reversed behind the pad"""
    from dynamont_amd import bam_io
    from dynamont_amd.segmentation.segment import POLYA, batch_site_ids
    from dynamont_amd.sites import contig_offsets
    tags = dict(qs=12.5, ns=5000, ts=10, fn="reads.pod5", sm=90.0, sd=15.0)
    seq = "ACGTACGTAC"
    m = lambda c: [n << 4 | "MIDNSHP=X".index(o) for n, o in c]  # noqa: E731
    recs = [("fwd", seq, tags, (0, 1, 7, m([(2, "S"), (8, "M")]))), ("unmapped", seq, tags, (4, -1, -1, [])),
            ("secondary", seq, tags, (256, 0, 1, m([(10, "M")]))), ("supplementary", seq, tags, (2048, 0, 1, m([(10, "M")]))),
            ("reverse", seq, tags, (16, 0, 1, m([(10, "M")]))), ("cg_tag", seq, tags, (0, 0, 1, m([(10, "S"), (30, "N")]))),
            ("short_cigar", seq, tags, (0, 0, 1, m([(9, "M")]))), ("fwd0", seq, tags, (0, 0, 0, m([(10, "="),])))]
    path = str(tmp_path / "m.bam")
    bam_io.write_bam(path, recs, references=[("chrA", 50), ("chrB", 40)])
    offs = contig_offsets([50, 40])
    for rna in (False, True):
        rd = bam_io.NativeBamJobs(path, rna=rna, pad=POLYA)
        jb = rd.next(100)
        ids, without = batch_site_ids(jb, rd.alignment(), offs, rna)
        rd.close()
        assert without == 6 and [len(i) for i in ids] == np.diff(jb.seq_off.astype(np.int64)).tolist()
        for k in range(1, 7):
            assert (ids[k] == ssc.NONE).all(), k
        fwd, fwd0 = [ssc.NONE] * 2 + list(range(57, 65)), list(range(0, 10))
        if rna:
            assert ids[0].tolist() == [ssc.NONE] * 9 + fwd[::-1] and ids[7].tolist() == [ssc.NONE] * 9 + fwd0[::-1]
        else:
            assert ids[0].tolist() == fwd and ids[7].tolist() == fwd0
        jb.site_ids = ids
        assert [i.tolist() for i in jb.take(np.array([0, 7])).site_ids] == [ids[0].tolist(), ids[7].tolist()]


HAND_SITES = {  # site -> (n_rows, n_samples, dwell_sq, M1, M2); two contigs of 5 and 4 positions
    1: (2, 30, 500, 3 << 40, (25 * 4 + 49 * 4) << 34),                 # means 1.25 and 1.75, dwells 10 and 20
    5: (1, 7, 49, -(2 << 40), 4 << 40),                                 # one read, mean -2: both spreads are 0
    8: (3, 3 + (1 << 33), (1 << 66) % (1 << 64) + 2, -(1 << 71) - 12345, (1 << 103) + 7),   # past the limbs
    4: (5, 11, 29, 1, 0),                                               # a negative variance in exact arithmetic: taken as 0
}


def test_tsv_writer_against_the_formulas(tmp_path):
    import math
    from dynamont_amd.segmentation.utils import SITE_SUMMARY_HEADER, site_summary_row, write_site_summary
    from dynamont_amd.sites import contig_offsets
    acc = ssc.empty(9)
    for s, (n, ns, dq, m1, m2) in HAND_SITES.items():
        acc["n_rows"][s], acc["n_samples"][s], acc["dwell_sq"][s], acc["M1"][s], acc["M2"][s] = n, ns, dq, m1, m2
    full = site_summary_from_limbs(*ssc.limbs(acc))

    def fetch(lo, hi):                                               # what Aligner.site_summary(lo, hi) returns
        return {k: (v[lo:hi] if k not in ("limbs", "totals") else v) for k, v in full.items()}

    out = str(tmp_path / "s.tsv")
    assert write_site_summary(out, fetch, 9, ["chrA", "chrB"], contig_offsets([5, 4]), window=4) == 4    # three windows
    lines = open(out).read().split("\n")
    assert lines[0] + "\n" == SITE_SUMMARY_HEADER == "contig\tposition\tcoverage\tn_samples\tdwell_mean\tdwell_sd\tlevel_mean\tlevel_sd\n"
    assert lines[-1] == "" and len(lines) == 6
    assert lines[1] == "chrA\t2\t2\t30\t15.0\t5.0\t1.5\t0.25"            # reference order, positions 1-based
    assert lines[2].split("\t")[:4] == ["chrA", "5", "5", "11"] and lines[2].split("\t")[7] == "0.0"
    assert lines[3] == "chrB\t1\t1\t7\t7.0\t0.0\t-2.0\t0.0"
    for ln, s in zip(lines[1:5], (1, 4, 5, 8)):
        n, ns, dq, m1, m2 = HAND_SITES[s]
        dq %= 1 << 64
        p = ln.split("\t")
        lm = Fraction(m1, n * (1 << 40))
        lv = Fraction(m2, n * (1 << 40)) - lm ** 2
        dm = Fraction(ns, n)
        dv = Fraction(dq, n) - dm ** 2
        want = (float(dm), math.sqrt(max(0.0, float(dv)) if dv > 0 else 0.0), float(lm), math.sqrt(float(lv)) if lv > 0 else 0.0)
        assert tuple(float(x) for x in p[4:]) == want == site_summary_row(n, ns, dq, m1, m2), s
        assert p[4:] == [repr(x) for x in want] and (int(p[2]), int(p[3])) == (n, ns)
    assert float(lines[4].split("\t")[6]) < -2.0 ** 29
