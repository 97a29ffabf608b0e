"""CPU: the two-sample comparison of the per-site histograms and the exact add (dyn_aligner_site_compare,
dyn_aligner_site_summary_add). The restatement of tests/site_compare_cases.py against hand-worked sites, the bound between the binned
and the exact Kolmogorov-Smirnov distance, the header and the refusals of a handle without a device, the host helpers (site_welch,
ks_two_sample_p, save_site_table / load_site_table, write_site_summary's new argument), the refusals of --site-control before
anything starts, and the kernels' footprint from the cross-compiled code."""
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import site_compare_cases as scc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native as N
from dynamont_amd._dynamont import int128_of_limbs, limbs_of_int128, site_summary_from_limbs
from dynamont_amd.segmentation import utils

pytestmark = pytest.mark.usefixtures("native_lib")

SYMBOLS = ("dyn_aligner_site_summary_add", "dyn_aligner_site_compare")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    c = scc.compare
    assert c([2, 1, 0, 3], [2, 1, 0, 3]) == (6, 6, 0, 0, 0)                       # identical: num 0 at the first counter, no side
    assert c([4, 2, 0, 6], [2, 1, 0, 3]) == (12, 6, 0, 0, 0)                      # ... the same SHAPE is identical too
    assert c([3, 2, 0, 0], [0, 0, 1, 3]) == (5, 4, 20, 1, 1)                      # disjoint: nA * nB, where A has ended
    assert c([0, 0, 1, 3], [3, 2, 0, 0]) == (4, 5, 20, 1, -1)
    # a tie between two counters: PA = 1 1 2 2 2, PB = 0 2 2 2 2 (n = 2 each): d = 2 at counter 0 (A ahead) and at 1 (B ahead)
    assert c([1, 0, 1, 0, 0], [0, 2, 0, 0, 0]) == (2, 2, 2, 0, 1)
    assert c([1, 0, 1, 0, 0], [0, 2, 0, 0, 0], tie="largest") == (2, 2, 2, 1, -1)
    # the maximum at the under counter; in the last interior bin (bins = 3: counter 3; counter 4, over, always has d = 0)
    assert c([5, 1, 1, 1, 0], [0, 3, 3, 2, 0]) == (8, 8, 40, 0, 1)
    assert c([0, 0, 0, 0, 4], [1, 1, 1, 1, 0]) == (4, 4, 16, 3, -1)
    # x = PA * nB against y = PB * nA with unequal totals: PA = 1 3 3, PB = 2 2 6: x = 6 18 18, y = 6 6 18
    assert c([1, 2, 0], [2, 0, 4]) == (3, 6, 12, 1, 1)
    # an empty side
    assert c([0, 0, 0], [1, 2, 3]) == (0, 6, 0, scc.NO_AT, 0) and c([1, 2, 3], [0, 0, 0]) == (6, 0, 0, scc.NO_AT, 0)
    assert c([0, 0], [0, 0]) == (0, 0, 0, scc.NO_AT, 0)
    top = 2 ** 32 - 1
    assert c([top, 0, 0], [0, 0, top]) == (top, top, top * top, 0, 1) and top * top < 2 ** 64
    pair = scc.compare_pair([1, 0, 1, 0, 0], [3] + [0] * 15, [0, 2, 0, 0, 0], [0] * 15 + [1])
    assert pair == dict(n_a=2, n_b=2, level_num=2, level_at=0, level_side=1, dwell_num=3, dwell_at=0, dwell_side=1)
    # the add: mod 2^64, mod 2^128 with the carry, two's complement
    M = 2 ** 64
    assert scc.add_cell([M - 1, 5, M - 3, M - 4, 6, 1000, 0], [2, 6, 10, 10, 0, *scc.limbs(-12345)]) == [1, 11, 7, 6, 7, M - 11345, M - 1]
    assert scc.add_counters([0xFFFFFFF0, 1], [0x20, 2]) == [0x10, 3]
    lo, hi = limbs_of_int128([-12345, 1 << 100, 0, -(1 << 127)])
    assert (int(lo[0]), int(hi[0])) == scc.limbs(-12345) and int128_of_limbs(lo, hi).tolist() == [-12345, 1 << 100, 0, -(1 << 127)]


def test_harness_tables_hold_the_cases_and_tell_a_wrong_tie_rule_apart():
    for w, t in scc.compare_tables().items():
        level, dwell = scc.split(t, w)
        assert max(sum(r) for r in level) < 2 ** 32 and max(sum(r) for r in dwell) < 2 ** 32          # the defined domain
        right = scc.compare_arrays(level, dwell, *scc.WINDOWS[0])
        wrong = scc.compare_arrays(level, dwell, *scc.WINDOWS[0], tie="largest")
        i = scc.BUILT.index("tie")
        assert (right["level_at"][i], right["level_side"][i]) == (0, 1) and (wrong["level_at"][i], wrong["level_side"][i]) == (w - 3, -1)
        assert right["level_at"][scc.BUILT.index("last")] == w - 2 and right["level_at"][scc.BUILT.index("round0")] == 0
        assert int(right["level_num"][scc.BUILT.index("top")]) == (2 ** 32 - 1) ** 2
        for name in ("empty_a", "empty_b", "empty_both"):
            assert right["level_at"][scc.BUILT.index(name)] == scc.NO_AT and right["dwell_at"][scc.BUILT.index(name)] == scc.NO_AT
        assert len({int(v) for v in right["level_at"]}) >= min(w, 6)                                       # the seeded pairs spread the argmax
        rounds = {int(v) // 64 for v in right["level_at"] if v != scc.NO_AT}
        assert rounds == set(range((w + 63) // 64))                                                   # a maximum in every round


@pytest.mark.parametrize("spec", [(32, -4.0, 4.0), (30, -3.3, 4.1)], ids=["32", "30"])
def test_binned_ks_bounds_the_exact_one(spec):
    """D_binned <= D_raw <= D_binned + max bin share on 200 seeded pairs of raw samples: the distribution functions are compared at
    the bin edges only, and inside a bin one of them has grown by at most its bin share since the edge"""
    rng = np.random.default_rng(4242)
    strict = 0
    for k in range(200):
        n_a, n_b = int(rng.integers(1, 120)), int(rng.integers(1, 120))
        xs = rng.normal(rng.normal(0, 1), rng.uniform(0.1, 2.0), n_a).tolist()
        ys = rng.normal(rng.normal(0, 1), rng.uniform(0.1, 2.0), n_b).tolist()
        if k % 10 == 0:
            ys = ys + xs[:n_a // 2]                                      # shared values: ties between the samples
        a, b = scc.binned(xs, *spec), scc.binned(ys, *spec)
        assert sum(a) == len(xs) > 0 and sum(b) == len(ys) > 0           # no pair is excluded for emptiness
        _, _, num, at, _ = scc.compare(a, b)
        raw, den = scc.ks_exact(xs, ys)
        assert den == sum(a) * sum(b)
        assert num <= raw and Fraction(raw, den) <= Fraction(num, den) + scc.bin_share(a, b), (k, num, raw, den)
        strict += num < raw
    assert strict > 50                                                   # the binned statistic does fall short, and often


# ---- header and handle -------------------------------------------------------------------------------------------------------------
def test_header_text_and_symbols(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION (\d+)\b", hdr).group(1) == "10"        # added within ABI 10
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    flat = " ".join(hdr.split())
    assert ("int dyn_aligner_site_summary_add(dyn_aligner* a, uint64_t lo, uint64_t hi, const uint64_t* n_rows, const uint64_t* n_samples, "
            "const uint64_t* dwell_sq, const uint64_t* m1_lo, const uint64_t* m1_hi, const uint64_t* m2_lo, const uint64_t* m2_hi, "
            "const uint64_t totals[5], /* may be NULL: adds none */ const uint32_t* level, const uint32_t* dwell);") in flat
    assert ("int dyn_aligner_site_compare(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint64_t other_lo, uint32_t* n_a, "
            "uint32_t* n_b, uint64_t* level_num, uint32_t* level_at, int32_t* level_side, uint64_t* dwell_num, uint32_t* dwell_at, "
            "int32_t* dwell_side);") in flat
    assert "site_compare_kernels.hpp" in N.HEADERS and "site_summary.hip" in N.SOURCES
    stubs = open(os.path.join(ROOT, "tools", "sanitize", "kernel_stubs.cpp")).read()
    assert "void launch_site_compare(const SiteCompare&, hipStream_t)" in stubs and "void launch_site_add(const SiteAdd&, hipStream_t)" in stubs


def test_a_handle_without_a_device_and_null_handles(native_lib, models):
    """the argument checks come before the device is looked at: the same text with or without one"""
    assert native_lib.dyn_aligner_site_summary_add(None, 0, 0, *[None] * 10) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_compare(None, 0, 0, 0, *[None] * 8) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")
    one = {"n_rows": [1], "n_samples": [3], "dwell_sq": [9], "M1": [-5], "M2": [7]}
    u64 = np.zeros(1, dtype=np.uint64)
    u32 = np.zeros(34, dtype=np.uint32)
    p64, p32 = u64.ctypes.data_as(N.c_u64_p), u32.ctypes.data_as(N.c_u32_p)
    for level, dwell in ((p32, None), (None, p32)):
        assert native_lib.dyn_aligner_site_summary_add(al._h, 0, 1, *[p64] * 7, None, level, dwell) == N.DYN_ERR_INVALID_ARGUMENT
        assert "dyn_aligner_site_summary_add: level and dwell counters are given together or not at all" in al.last_error()
    assert native_lib.dyn_aligner_site_summary_add(al._h, 0, 1, p64, None, *[p64] * 5, None, None, None) == N.DYN_ERR_INVALID_ARGUMENT   # a NULL column
    assert native_lib.dyn_aligner_site_compare(al._h, 0, 1, 0, *[None] * 8) == N.DYN_ERR_INVALID_ARGUMENT                            # NULL outputs
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_summary_add(0, one)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_compare(0, 0, 0)
    with pytest.raises(ValueError, match="differ in length"):
        al.site_summary_add(0, dict(one, M1=[1, 2]))
    al.close()
    with pytest.raises(NotImplementedError, match=r"MultiAligner has no per-site summary \(Aligner.site_summary_add\): use one Aligner per device"):
        MultiAligner.site_summary_add(None, 0, one)
    with pytest.raises(NotImplementedError, match=r"MultiAligner has no per-site histograms \(Aligner.site_compare\): use one Aligner per device"):
        MultiAligner.site_compare(None)


def test_kernels_compile_with_the_products_flags_beside_a_resident_workgroup(tmp_path):
    """tests/device_math/site_compare.hip builds with the product's flags; the compiler's resource remarks show every width of the
    comparison kernel and the add kernel without scratch, without LDS and within 152 VGPRs"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "site_compare.hip"), "-o", str(tmp_path / "libsc.so")]
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == 6 and sum("k_site_compare" in n for n in names) == 5 and sum("k_site_add" in n for n in names) == 1
    assert scratch == [0] * 6 and lds == [0] * 6 and max(vgprs) <= 152, (scratch, lds, vgprs)


# ---- host helpers --------------------------------------------------------------------------------------------------------------------
def row_of(values):
    """(n_rows, M1, M2) of event means that are multiples of 2^-40"""
    return len(values), sum(int(v * 2 ** 40) for v in values), sum(int(v * v * 2 ** 40) for v in values)


def test_site_welch_by_hand():
    # A = 1, 2, 3 (mean 2, var 1), B = 4, 6 (mean 5, var 2): se^2 = 1/3 + 1 = 4/3, t = -3 / sqrt(4/3), df = (16/9) / (1/18 + 1) = 32/19
    t, df = utils.site_welch(row_of([1.0, 2.0, 3.0]), row_of([4.0, 6.0]))
    assert t == -math.sqrt(float(Fraction(27, 4))) and df == float(Fraction(32, 19))
    t2, df2 = utils.site_welch(row_of([4.0, 6.0]), row_of([1.0, 2.0, 3.0]))
    assert (t2, df2) == (-t, df)
    # equal variances and sizes: df = 2 n - 2
    t, df = utils.site_welch(row_of([0.5, 1.5, 0.5, 1.5]), row_of([2.5, 3.5, 2.5, 3.5]))
    assert df == 6.0 and t == -math.sqrt(float(Fraction(4) / (Fraction(1, 3) / 4 * 2)))
    for a, b in ((row_of([1.0]), row_of([1.0, 2.0])), (row_of([1.0, 2.0]), row_of([3.0])), ((0, 0, 0), row_of([1.0, 2.0])),
                 (row_of([2.0, 2.0]), row_of([3.0, 3.0, 3.0]))):            # fewer than 2 rows; a standard error of 0
        assert all(math.isnan(v) for v in utils.site_welch(a, b))
    t, df = utils.site_welch(row_of([2.0, 2.0]), row_of([3.0, 4.0]))       # one side without spread: df is the other side's
    assert df == 1.0 and t == -math.sqrt(float(Fraction(9, 4) / Fraction(1, 4)))


def test_ks_two_sample_p():
    p = utils.ks_two_sample_p
    assert p(0.0, 50, 60) == 1.0 and p(1.0, 10 ** 6, 10 ** 6) < 1e-12 and 0.0 <= p(1.0, 3, 3) <= 1.0
    ds = np.linspace(0.0, 1.0, 201)
    ps = [p(float(d), 40, 55) for d in ds]
    # monotone in d up to the rounding of the alternating sum: at most 1 / 0.04 * sqrt(18.4) = 108 terms (the function sums down to
    # lam = 0.04), each partial sum rounded to half an ulp of 1, doubled: 108 * 2^-53 * 2 < 1e-13
    assert all(a >= b - 1e-13 for a, b in zip(ps, ps[1:])) and ps[0] == 1.0 and ps[-1] < 1e-8
    assert all(a > b for a, b in zip(ps[20:], ps[21:]))               # ... and strictly once p has left 1
    assert math.isnan(p(math.nan, 5, 5)) and math.isnan(p(0.5, 0, 5))
    # lam = 1: 2 (e^-2 - e^-8 + e^-18 - e^-32 + ...)
    ne = 40 * 55 / 95
    d = 1.0 / (math.sqrt(ne) + 0.12 + 0.11 / math.sqrt(ne))
    assert abs(p(d, 40, 55) - 2 * (math.exp(-2) - math.exp(-8) + math.exp(-18) - math.exp(-32))) < 1e-15
    assert "conservative" in p.__doc__


def test_ks_two_sample_p_against_scipy():
    try:
        from scipy.stats import kstwobign
    except ImportError:
        pytest.skip("scipy is not importable here: the comparison with scipy.stats.kstwobign is left out")
    n = 10 ** 6
    ne = n * n / (2 * n)
    f = math.sqrt(ne) + 0.12 + 0.11 / math.sqrt(ne)
    for lam in np.concatenate([np.linspace(0.01, 3.0, 300), [0.04, 0.0401, 5.0, 8.0]]).tolist():
        assert abs(utils.ks_two_sample_p(lam / f, n, n) - float(kstwobign.sf(f * (lam / f)))) < 1e-12, lam


class StubAligner:
    """site_summary / site_histogram / site_summary_add over host arrays, shaped like Aligner's"""

    def __init__(self, n, spec=None):
        self.cols = [np.zeros(n, dtype=np.uint64) for _ in range(7)]
        self.totals = np.zeros(5, dtype=np.uint64)
        self._site_histogram = spec
        self.level = np.zeros((n, spec[0] + 2), dtype=np.uint32) if spec else None
        self.dwell = np.zeros((n, 16), dtype=np.uint32) if spec else None
        self.windows = []

    def site_summary(self, lo=0, hi=None):
        self.windows.append((lo, hi))
        return site_summary_from_limbs([c[lo:hi] for c in self.cols], self.totals)

    def site_histogram(self, lo=0, hi=None):
        return {"level": self.level[lo:hi], "dwell": self.dwell[lo:hi]}

    def site_summary_add(self, lo, summary, histogram=None):
        n = len(summary["n_rows"])
        for f, k in enumerate(("n_rows", "n_samples", "dwell_sq")):
            self.cols[f][lo:lo + n] += np.asarray(summary[k], dtype=np.uint64)
        for f, k in ((3, "M1"), (5, "M2")):
            old = int128_of_limbs(self.cols[f][lo:lo + n], self.cols[f + 1][lo:lo + n])
            self.cols[f][lo:lo + n], self.cols[f + 1][lo:lo + n] = limbs_of_int128([int(a) + int(b) for a, b in zip(old, summary[k])])
        if histogram is not None:
            self.level[lo:lo + n] += histogram["level"]
            self.dwell[lo:lo + n] += histogram["dwell"]


def filled_stub(n, spec, seed, covered):
    rng = np.random.default_rng(seed)
    st = StubAligner(n, spec)
    for s in covered:
        st.cols[0][s], st.cols[1][s], st.cols[2][s] = rng.integers(1, 50), rng.integers(50, 500), rng.integers(500, 5000)
    m1 = [0] * n
    for s in covered:
        m1[s] = -int(rng.integers(1, 1 << 62)) * (1 << 10)               # negative M1: the high limb is all ones
    st.cols[3], st.cols[4] = limbs_of_int128(m1)
    st.cols[5][list(covered)] = rng.integers(1, 1 << 62, len(covered)).astype(np.uint64)
    if spec:
        for s in covered:
            st.level[s] = rng.integers(0, 9, spec[0] + 2)
            st.dwell[s] = rng.integers(0, 9, 16)
    st.totals[:] = [5, 40, 400, 3, 1]
    return st, m1


@pytest.mark.parametrize("spec", [None, (30, -3.3, 4.1)], ids=["table", "histograms"])
def test_site_table_round_trip(tmp_path, spec):
    n, covered = 1000, [0, 3, 4, 255, 256, 700, 999]
    st, m1 = filled_stub(n, spec, 5, covered)
    path = str(tmp_path / "t.npz")
    assert utils.save_site_table(path, st, ["c1", "c2"], [600, 400], window=256) == len(covered) and os.path.exists(path)
    assert st.windows == [(0, 256), (256, 512), (512, 768), (768, 1000)]      # window by window
    t = utils.load_site_table(path)
    assert t["version"] == 1 and t["num_sites"] == n and t["site"].tolist() == covered and t["ref_names"] == ["c1", "c2"]
    assert t["ref_lengths"].tolist() == [600, 400] and t["totals"] == dict(reads_ok=5, rows_added=40, samples_added=400, rows_without_site=3, rows_skipped=1)
    assert [int(v) for v in t["M1"]] == [m1[s] for s in covered] and all(v < 0 for v in t["M1"])
    for f in range(7):
        assert np.array_equal(t["limbs"][f], st.cols[f][covered])
    if spec:
        assert t["hist_spec"] == spec and np.array_equal(t["level"], st.level[covered]) and np.array_equal(t["dwell"], st.dwell[covered])
        assert t["hist_bits"].tolist() == [30] + np.array(spec[1:]).view(np.uint64).tolist()
    else:
        assert t["hist_spec"] is None and t["level"] is None and t["dwell"] is None
    # back onto a table of 2 n sites, into the second half
    back = StubAligner(2 * n, spec)
    assert utils.load_site_control(back, t, n, window=300) == len(covered)
    for f in range(7):
        assert not back.cols[f][:n].any() and np.array_equal(back.cols[f][n:], st.cols[f])
    assert not back.totals.any()                                          # the handle's totals stay the run's own
    if spec:
        assert np.array_equal(back.level[n:], st.level) and np.array_equal(back.dwell[n:], st.dwell)
    # a window of the table; an empty table
    assert utils.save_site_table(path, st, ["c1", "c2"], [600, 400], lo=200, hi=800) == 3
    assert utils.load_site_table(path)["site"].tolist() == [55, 56, 500] and utils.load_site_table(path)["num_sites"] == 600
    empty = StubAligner(10, spec)
    assert utils.save_site_table(path, empty, ["c"], [10]) == 0
    t = utils.load_site_table(path)
    assert t["site"].size == 0 and t["M1"].size == 0 and (t["level"].shape == (0, 32) if spec else t["level"] is None)
    assert utils.load_site_control(StubAligner(20, spec), t, 10) == 0
    with np.load(path) as z:
        other = {k: z[k] for k in z.files}
    other["version"] = np.array([2], dtype=np.uint32)
    np.savez(str(tmp_path / "v2.npz"), **other)
    with pytest.raises(ValueError, match="format version 2"):
        utils.load_site_table(str(tmp_path / "v2.npz"))


# ---- dynamont-resquiggle --site-table-out / --site-control ---------------------------------------------------------------------------
def test_cli_flags_and_refusals_before_anything_starts(models, tmp_path, monkeypatch):
    """no aligner, no output file: --site-control without --site-histogram, references that differ in name or length, a file
    without histograms, a hist_spec that differs in the last bit"""
    from dynamont_amd import bam_io
    from dynamont_amd.segmentation import segment as seg
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).site_control == "" and seg.parse(base).site_table_out == ""
    args = seg.parse(base + ["--site-summary", "s.tsv", "--site-histogram", "32:-4:4", "--site-control", "c.npz", "--site-table-out", "t.npz"])
    assert (args.site_control, args.site_table_out) == ("c.npz", "t.npz")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    tags = dict(qs=12.5, ns=5000, ts=10, fn="reads.pod5", sm=90.0, sd=15.0)
    mapped = str(tmp_path / "m.bam")
    bam_io.write_bam(mapped, [("r0", "ACGTACGTACGT", dict(tags), (0, 0, 3, [12 << 4]))], references=[("chrA", 100), ("chrB", 50)])
    out, tsv = str(tmp_path / "out.csv.zst"), str(tmp_path / "s.tsv")
    run = lambda **kw: seg.segment(str(tmp_path), mapped, 1, out, models["syn9"], "rna004", "basic", **kw)  # noqa: E731
    spec = (32, -4.0, 4.0)
    st, _ = filled_stub(150, spec, 9, [1, 2, 120])
    good, names_differ, lengths_differ, no_hist, last_bit = (str(tmp_path / f) for f in ("good.npz", "names.npz", "len.npz", "nohist.npz", "bit.npz"))
    utils.save_site_table(good, st, ["chrA", "chrB"], [100, 50])
    utils.save_site_table(names_differ, st, ["chrA", "chrC"], [100, 50])
    utils.save_site_table(lengths_differ, st, ["chrA", "chrB"], [101, 49])
    utils.save_site_table(no_hist, filled_stub(150, None, 9, [1, 2, 120])[0], ["chrA", "chrB"], [100, 50])
    st._site_histogram = (32, -4.0, float(np.nextafter(4.0, 5.0)))
    utils.save_site_table(last_bit, st, ["chrA", "chrB"], [100, 50])
    with pytest.raises(ValueError, match="--site-control compares the per-site histograms of the run and the control: it needs --site-summary FILE and"):
        run(site_summary=tsv, site_control=good)
    with pytest.raises(ValueError, match="--site-control compares"):
        run(site_control=good)
    with pytest.raises(ValueError, match="--site-table-out saves the per-site table: it needs --site-summary FILE"):
        run(site_table_out=str(tmp_path / "t.npz"))
    hist = dict(site_summary=tsv, site_histogram="32:-4:4")
    with pytest.raises(ValueError, match="its reference names differ from the BAM header's"):
        run(site_control=names_differ, **hist)
    with pytest.raises(ValueError, match="its reference lengths differ from the BAM header's"):
        run(site_control=lengths_differ, **hist)
    with pytest.raises(ValueError, match="the file holds no histograms"):
        run(site_control=no_hist, **hist)
    with pytest.raises(ValueError, match=r"are not the run's \(32 bins over \[-4.0, 4.0\)\), bit for bit"):
        run(site_control=last_bit, **hist)
    with pytest.raises(ValueError, match=r"are not the run's \(30 bins"):
        run(site_control=good, site_summary=tsv, site_histogram="30:-4:4")
    utils.check_site_control(utils.load_site_table(good), good, ["chrA", "chrB"], [100, 50], spec)        # the good one passes ...
    utils.check_site_control(utils.load_site_table(good), good, ["chrA", "chrB"], [100, 50], (32, None, None))   # ... a range still unknown too
    assert not os.path.exists(out) and not os.path.exists(tsv) and not os.path.exists(tmp_path / "t.npz")


def test_tsv_writer_with_a_control(tmp_path):
    """without the new argument: the bytes it wrote before, on a stub table; with it: the header and one worked line"""
    n = 6
    cols = {"n_rows": np.array([0, 2, 0, 1, 0, 3], dtype=np.uint64), "n_samples": np.array([0, 9, 0, 4, 0, 30], dtype=np.uint64),
            "dwell_sq": np.array([0, 41, 0, 16, 0, 300], dtype=np.uint64),
            "M1": np.array([0, 3 << 40, 0, -(1 << 39), 0, 0], dtype=object), "M2": np.array([0, 5 << 40, 0, 1 << 38, 0, 0], dtype=object)}
    fetch = lambda lo, hi: {k: v[lo:hi] for k, v in cols.items()}  # noqa: E731
    offs = np.array([0, 4, 6])
    plain, with_c = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    assert utils.write_site_summary(plain, fetch, n, ["c1", "c2"], offs, window=4) == 3
    want = ("contig\tposition\tcoverage\tn_samples\tdwell_mean\tdwell_sd\tlevel_mean\tlevel_sd\n"
            "c1\t2\t2\t9\t4.5\t0.5\t1.5\t0.5\nc1\t4\t1\t4\t4.0\t0.0\t-0.5\t0.0\nc2\t2\t3\t30\t10.0\t0.0\t0.0\t0.0\n")
    assert open(plain).read() == want
    # the control: site 1 against values 1, 2, 2 (the run holds 1 and 2: M1 = 3, M2 = 5), sites 3 and 5 against nothing
    ctl = {"n_rows": np.array([0, 3, 0, 0, 0, 0]), "M1": np.array([0, 5 << 40, 0, 0, 0, 0], dtype=object),
           "M2": np.array([0, 9 << 40, 0, 0, 0, 0], dtype=object)}
    comp = {"n_a": np.array([0, 2, 0, 1, 0, 3], dtype=np.uint32), "n_b": np.array([0, 3, 0, 0, 0, 0], dtype=np.uint32),
            "level_d": np.array([np.nan, 1 / 6, np.nan, np.nan, np.nan, np.nan]), "dwell_d": np.array([np.nan, 0.5, np.nan, np.nan, np.nan, np.nan]),
            "level_edge": np.array([np.nan, 1.25, np.nan, np.nan, np.nan, np.nan]), "level_side": np.array([0, 1, 0, 0, 0, 0], dtype=np.int32)}
    calls = []

    def control(lo, hi, run):
        calls.append((lo, hi))
        assert np.array_equal(run["n_rows"], cols["n_rows"][lo:hi])          # the window write_site_summary fetched
        return utils.site_control_columns({k: v[lo:hi] for k, v in comp.items()}, run, {k: v[lo:hi] for k, v in ctl.items()})
    assert utils.write_site_summary(with_c, fetch, n, ["c1", "c2"], offs, window=4, control=control) == 3
    assert calls == [(0, 4), (4, 6)]
    got = open(with_c).read().splitlines()
    assert got[0] == want.splitlines()[0] + "\tcontrol_coverage\tks_d\tks_p\tks_level\tks_side\tdwell_ks_d\twelch_t\twelch_df"
    assert [x.split("\t")[:8] for x in got] == [x.split("\t") for x in want.splitlines()]
    # the run: mean 3/2, unbiased var 1/2; the control: mean 5/3, var 1/3: se^2 = 1/4 + 1/9 = 13/36, t = -(1/6) / sqrt(13/36),
    # df = (13/36)^2 / ((1/16) / 1 + (1/81) / 2)
    t = -math.sqrt(float(Fraction(1, 36) / Fraction(13, 36)))
    df = float(Fraction(13, 36) ** 2 / (Fraction(1, 16) + Fraction(1, 162)))
    assert got[1].split("\t")[8:] == ["3", repr(1 / 6), repr(utils.ks_two_sample_p(1 / 6, 2, 3)), "1.25", "1", "0.5", repr(t), repr(df)]
    assert got[2].split("\t")[8:] == ["0", "nan", "nan", "nan", "0", "nan", "nan", "nan"] == got[3].split("\t")[8:]
