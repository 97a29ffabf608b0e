"""CPU: the per-site histograms and quantiles (dyn_aligner_set_site_histogram, dyn_aligner_site_histogram_fetch,
dyn_aligner_site_quantiles). The restatement of tests/site_histogram_cases.py against hand-worked values, the harness inputs
against every wrong version the restatement can be told from, the header and the refusals of a handle without a device, the
host quantile formula, the --site-histogram parser and its refusal without --site-summary, and the kernels' footprint from the
cross-compiled code."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import site_histogram_cases as shc
import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native as N
from dynamont_amd.segmentation import utils

pytestmark = pytest.mark.usefixtures("native_lib")

SYMBOLS = ("dyn_aligner_set_site_histogram", "dyn_aligner_site_histogram_fetch", "dyn_aligner_site_quantiles")


# ---- header and handle -----------------------------------------------------------------------------------------------------------
def test_header_text_and_symbols(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION (\d+)\b", hdr).group(1) == "10"        # added within ABI 10
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    flat = " ".join(hdr.split())
    assert "int dyn_aligner_set_site_histogram(dyn_aligner* a, int bins, double lo, double hi);" in flat
    assert ("int dyn_aligner_site_histogram_fetch(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, uint32_t* level, "
            "uint32_t* dwell);") in flat
    assert ("int dyn_aligner_site_quantiles(dyn_aligner* a, uint64_t site_lo, uint64_t site_hi, const double* probs, int n_probs, "
            "uint32_t* n, uint32_t* rank, uint32_t* bin, uint32_t* below, uint32_t* in_bin);") in flat


def test_a_handle_without_a_device_refuses_with_the_devices_texts(native_lib, models):
    """the argument checks and the missing table come before the device is looked at: the same text with or without one
    (tests/test_gpu_site_histogram.py asks a device handle for the same texts)"""
    assert native_lib.dyn_aligner_set_site_histogram(None, 32, -4.0, 4.0) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_histogram_fetch(None, 0, 0, None, None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_quantiles(None, 0, 0, None, 1, None, None, None, None, None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_histogram: dyn_aligner_set_site_summary\(a, num_sites > 0\) was never called on this handle"):
        al.set_site_histogram(32, -4.0, 4.0)
    for bins in (1, 255, -3):
        with pytest.raises(ValueError, match=r"bins %d is not 0 \(off\) or 2 \.\. 254" % bins):
            al.set_site_histogram(bins, -4.0, 4.0)
    for lo, hi in ((4.0, 4.0), (4.0, -4.0), (math.nan, 4.0), (-4.0, math.nan), (-math.inf, 4.0), (-4.0, math.inf)):
        with pytest.raises(ValueError, match="lo and hi must be finite with lo < hi"):
            al.set_site_histogram(32, lo, hi)
    with pytest.raises(ValueError, match=r"finite bins / \(hi - lo\)"):
        al.set_site_histogram(32, -1.7e308, 1.7e308)                 # hi - lo overflows: no width
    with pytest.raises(ValueError, match=r"finite bins / \(hi - lo\)"):
        al.set_site_histogram(32, 0.0, 5e-324)                       # 32 / a denormal overflows
    al.set_site_histogram(0)                                         # off is always fine
    assert al._site_histogram is None
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_histogram(0, 0)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_quantiles([0.5], 0, 0)
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities in \[0, 1\]"):
        al.site_quantiles([])
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities in \[0, 1\]"):
        al.site_quantiles([0.5] * 9)
    with pytest.raises(ValueError, match=r"1 \.\. 8 probabilities in \[0, 1\]"):
        al.site_quantiles([0.5, 1.5])
    q = np.array([0.5, math.nan])
    one = np.zeros(2, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(N.c_u32_p)  # noqa: E731
    assert native_lib.dyn_aligner_site_quantiles(al._h, 0, 1, q.ctypes.data_as(N.c_double_p), 2, p(one), p(one), p(one), p(one),
                                                 p(one)) == N.DYN_ERR_INVALID_ARGUMENT
    assert "probs[1] is not in [0, 1]" in al.last_error()
    assert native_lib.dyn_aligner_site_quantiles(al._h, 0, 1, q.ctypes.data_as(N.c_double_p), 9, p(one), p(one), p(one), p(one),
                                                 p(one)) == N.DYN_ERR_INVALID_ARGUMENT
    assert "n_probs 9 is not 1 .. 8" in al.last_error()
    al.close()
    with pytest.raises(NotImplementedError, match="MultiAligner has no per-site histograms"):
        MultiAligner.set_site_histogram(None, 32, -4.0, 4.0)


def test_sources_and_the_unchanged_initialisers():
    """the quantile kernel lives in a header of its own, so that the site summary's harness still holds two kernels; the aggregate
    initialisers of launch.cpp and of that harness stop at read_hi and leave the histogram fields zero (off)"""
    assert "site_quantile_kernels.hpp" in N.HEADERS and "site_summary.hip" in N.SOURCES
    ssk = open(os.path.join(N.CSRC, "site_summary_kernels.hpp")).read()
    assert "k_site_quantiles" not in ssk.split("#pragma once")[1] and "if (ss.hist)" in ssk
    launch = open(os.path.join(N.CSRC, "launch.cpp")).read()
    assert "totals, (uint32_t)b->ss_num_sites, 0u, (uint32_t)b->n}" in launch
    nt = open(os.path.join(N.CSRC, "nt_kernels.hpp")).read()
    body = nt[nt.index("struct SiteSummary {"):]
    body = body[:body.index("};")]
    assert body.index("read_lo, read_hi") < body.index("unsigned int* hist") < body.index("uint32_t bins") < body.index("double hist_lo, inv_w")
    stubs = open(os.path.join(ROOT, "tools", "sanitize", "kernel_stubs.cpp")).read()
    assert "void launch_site_quantiles(const SiteQuantiles&, hipStream_t)" in stubs


def test_kernels_compile_with_the_products_flags_beside_a_resident_workgroup(tmp_path):
    """tests/device_math/site_histogram.hip builds with the product's flags; the compiler's resource remarks show the two filling
    kernels and every width of the quantile kernel without scratch, within 13 KB of static LDS and 152 VGPRs (DESIGN.md section
    4), the quantile kernel without any LDS"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "site_histogram.hip"), "-o", str(tmp_path / "libsh.so")]
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == 7 and sum("k_ssum_" in n for n in names) == 2 and sum("k_site_quantiles" in n for n in names) == 5
    assert scratch == [0] * 7 and max(lds) <= 13 * 1024 and max(vgprs) <= 152, (scratch, lds, vgprs)
    assert all(l == 0 for n, l in zip(names, lds) if "k_site_quantiles" in n)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_restatement_by_hand():
    bins, lo, hi = shc.EXACT
    assert float(shc.inv_width(bins, lo, hi)) == 4.0
    lb = lambda m, how=None: shc.level_bin(m, bins, lo, hi, how)  # noqa: E731
    assert lb(-4.0) == 1 and lb(np.nextafter(-4.0, -np.inf)) == 0 and lb(-1e30) == 0
    # the double below 4: m - lo rounds to 8, so u == bins -- over, by the definition's own two operations (no comparison is made
    # against a nominal edge); the double below 3 is far enough from it
    assert lb(4.0) == 33 and lb(np.nextafter(4.0, 0.0)) == 33 and lb(1e30) == 33 and lb(3.99) == 32
    assert lb(0.0) == 17 and lb(-0.0) == 17 and lb(-5e-324) == 17 and lb(-1e-15) == 16 and lb(0.25) == 18 and lb(0.2499) == 17
    assert [shc.dwell_bin(L) for L in (1, 2, 3, 4, 7, 8, 32767, 32768, 40000, 1 << 20)] == [0, 1, 1, 2, 2, 3, 14, 15, 15, 15]
    # quantiles of [2 under | 1 | 0 | 3 | 0 over] (bins = 3): n = 6
    n, per = shc.quantiles([2, 1, 0, 3, 0], (0.0, 1e-12, 1 / 3, 0.5, 0.51, 1.0))
    assert n == 6
    assert per == [(1, 0, 0, 2), (1, 0, 0, 2), (2, 0, 0, 2), (3, 1, 2, 1), (4, 3, 3, 3), (6, 3, 3, 3)]
    assert shc.quantiles([0, 0, 0, 0], (0.5,)) == (0, [(0, shc.NO_BIN, 0, 0)])
    assert shc.quantiles([0, 0, 1, 0], (0.0, 1.0)) == (1, [(1, 2, 0, 1), (1, 2, 0, 1)])
    big = [3, 1 << 31, 5]
    assert shc.quantiles(big, (0.5, 1.0))[1] == [(((1 << 31) + 8) // 2, 1, 3, 1 << 31), ((1 << 31) + 8, 2, (1 << 31) + 3, 5)]


@pytest.fixture(scope="module")
def batch():
    return shc.build_batch()


def test_harness_batch_holds_the_cases(batch):
    lens = sorted({len(x) for _, segs in batch.reads for _, x in segs})
    for L in (1, 2, 3, 4, 63, 64, 65, 256, 257, 16384, 16392, 32767, 32768, 40000):
        assert L in lens
    assert len(shc.edge_neighbours()) == 527 and len(set(shc.edge_neighbours())) == 527
    assert len(shc.exact_edge_samples()) == 4 + 2 * 31
    for spec in (shc.EXACT, shc.ROUNDED):
        h = shc.reference(batch, *spec)
        t = ssc.reference(batch)
        for s in range(batch.num_sites):                              # both groups sum to the table's n_rows
            assert sum(h["level"][s]) == sum(h["dwell"][s]) == t["n_rows"][s], s
        assert t["totals"]["rows_without_site"] >= 4 and t["totals"]["rows_skipped"] >= 8
    h = shc.reference(batch, *shc.EXACT)
    row = h["level"][31]                                             # the 66 samples on the edges of (32, -4, 4)
    assert sum(row) == 66 and row[0] == 1 and row[33] == 2 and min(row[1:33]) >= 1 and max(row[1:33]) <= 3
    d = [sum(h["dwell"][s][b] for s in range(33, 39)) for b in range(16)]
    assert d[0] == 1 and d[1] == 2 and d[2] == 1 and d[14] == 1 and d[15] == 2
    assert sum(h["level"][11][1:33]) == 0 and h["level"][11][0] > 0 and h["level"][11][33] > 0   # levels of +-2^22: under and over


@pytest.mark.parametrize("how", ["float32", "rint", "clamped"])
def test_inputs_tell_a_wrong_binning_apart(batch, how):
    for spec in (shc.EXACT, shc.ROUNDED):
        right, wrong = shc.reference(batch, *spec), shc.reference(batch, *spec, how=how)
        assert right["level"] != wrong["level"], (how, spec)
        assert right["dwell"] == wrong["dwell"]
    if how == "float32":                                             # the 527 doubles around the edges of (30, -3.3, 4.1)
        v = shc.edge_neighbours()
        differ = sum(shc.level_bin(m, *shc.ROUNDED) != shc.level_bin(m, *shc.ROUNDED, how="float32") for m in v)
        assert differ > 100, differ


def test_two_rewritings_that_cannot_be_told_apart():
    """u > bins for u >= bins: the only u the two treat differently is u == bins, which the wrong one sends to 1 + int(bins) -- the
    over counter's own index. (m - lo) / w for (m - lo) * inv_w: no difference on the 527 edge neighbours nor on 50 000 random
    levels. Neither is listed as a wrong version that a test can catch."""
    rng = np.random.default_rng(3)
    for spec in (shc.EXACT, shc.ROUNDED):
        bins, lo, hi = spec
        vals = shc.edge_neighbours(spec) + shc.exact_edge_samples() + rng.normal(0.0, 3.0, 50000).tolist() + [hi, 1e300, -1e300]
        assert all(shc.level_bin(m, *spec) == shc.level_bin(m, *spec, how="gt") for m in vals)
        w = (np.float64(hi) - np.float64(lo)) / np.float64(bins)
        by_division = [min(max(1 + math.floor(float((np.float64(m) - np.float64(lo)) / w)), 0), bins + 1) for m in vals[:-2]]
        assert by_division == [shc.level_bin(m, *spec) for m in vals[:-2]]


@pytest.mark.parametrize("how", ["prefix_gt", "floor"])
def test_inputs_tell_a_wrong_quantile_rule_apart(how):
    for B, table in shc.quantile_tables().items():
        right = shc.quantile_arrays(table[:, :B].tolist(), shc.PROBS)
        wrong = shc.quantile_arrays(table[:, :B].tolist(), shc.PROBS, how=how)
        assert np.array_equal(right[0], wrong[0])
        assert any(not np.array_equal(a, b) for a, b in zip(right[1], wrong[1])), (how, B)
        if how == "prefix_gt":                                       # ... already on the site whose prefix sum meets k at a bin's end
            assert any(not np.array_equal(a[5], b[5]) for a, b in zip(right[1], wrong[1])), (how, B)


def test_a_row_stride_of_bins_reads_other_counters(batch):
    for spec in (shc.EXACT, shc.ROUNDED):
        h = shc.reference(batch, *spec)
        f = shc.flat(h)
        H = spec[0] + 2 + shc.DWELL_BINS
        assert f.size == batch.num_sites * H
        right = f.reshape(batch.num_sites, H)[:, :spec[0] + 2]
        assert np.array_equal(right, np.array(h["level"], dtype=np.uint32))
        assert not np.array_equal(right, shc.wrong_stride_level(f, batch.num_sites, spec[0]))


def test_quantile_tables_hold_the_cases():
    for B, t in shc.quantile_tables().items():
        lv = t[:, :B].astype(np.int64)
        assert lv[0].sum() == 0 and lv[3].sum() == 0 and lv[1, 0] == lv[1].sum() > 0 and lv[2, B - 1] == lv[2].sum() > 0 and lv[4].sum() == 1
        assert lv[6].sum() > 1 << 31 and lv[7].sum() < 1 << 32 and lv[7].sum() >= (1 << 31) + (1 << 30)
        n, per = shc.quantiles(lv[5], (0.25, 0.5))
        assert [(k, below + in_bin) for k, _, below, in_bin in per] == [(1, 1), (2, 2)]      # the prefix sum equals k at the bin's end
        assert (t[:, B:] == 0xABCD0000).all()


# ---- the host formula ----------------------------------------------------------------------------------------------------------------
def test_host_quantile_formula():
    bins, lo, hi = 32, -4.0, 4.0
    rank = np.array([[3, 1, 7, 0, 2]], dtype=np.uint32)
    bin_ = np.array([[17, 0, 33, shc.NO_BIN, 32]], dtype=np.uint32)
    below = np.array([[2, 0, 6, 0, 0]], dtype=np.uint32)
    in_bin = np.array([[4, 5, 1, 0, 2]], dtype=np.uint32)
    lv = utils.site_quantile_levels(rank, bin_, below, in_bin, bins, lo, hi)
    assert lv.shape == (1, 5) and lv.dtype == np.float64
    assert lv[0, 0] == -4.0 + (16 + (3 - 2 - 0.5) / 4) * 0.25        # the first of four rows in [0, 0.25): an eighth into the bin
    assert lv[0, 1] == -math.inf and lv[0, 2] == math.inf and math.isnan(lv[0, 3])
    assert lv[0, 4] == -4.0 + (31 + 1.5 / 2) * 0.25 and 3.75 <= lv[0, 4] < 4.0
    # an interior value always lies inside its bin
    rng = np.random.default_rng(1)
    b = rng.integers(1, 31, 500)
    ib = rng.integers(1, 1000, 500)
    r = rng.integers(0, 5000, 500)
    k = r + 1 + (rng.random(500) * ib).astype(np.int64)
    out = utils.site_quantile_levels(k, b, r, ib, 30, -3.3, 4.1)
    w = (4.1 + 3.3) / 30
    assert (out >= -3.3 + (b - 1) * w - 1e-12).all() and (out <= -3.3 + b * w + 1e-12).all()
    assert utils.site_quantile_levels(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), 4, 0.0, 1.0).shape == (0, 3)


def test_tsv_writer_adds_three_columns_and_leaves_the_others(tmp_path):
    n = 6
    cols = {"n_rows": np.array([0, 2, 0, 1, 0, 3], dtype=np.uint64), "n_samples": np.array([0, 9, 0, 4, 0, 30], dtype=np.uint64),
            "dwell_sq": np.array([0, 41, 0, 16, 0, 300], dtype=np.uint64),
            "M1": np.array([0, 3 << 40, 0, -(1 << 39), 0, 0], dtype=object), "M2": np.array([0, 5 << 40, 0, 1 << 38, 0, 0], dtype=object)}
    fetch = lambda lo, hi: {k: v[lo:hi] for k, v in cols.items()}  # noqa: E731
    level = np.array([[np.nan] * 3, [-0.5, 0.125, 0.75], [np.nan] * 3, [-np.inf, 0.1, np.inf], [np.nan] * 3, [1.0, 2.0, 3.0]])
    calls = []

    def quant(lo, hi):
        calls.append((lo, hi))
        return {"level": level[lo:hi]}
    plain, with_q = str(tmp_path / "a.tsv"), str(tmp_path / "b.tsv")
    offs = np.array([0, 4, 6])
    assert utils.write_site_summary(plain, fetch, n, ["c1", "c2"], offs, window=4) == 3
    assert utils.write_site_summary(with_q, fetch, n, ["c1", "c2"], offs, window=4, quantiles=quant) == 3
    assert calls == [(0, 4), (4, 6)]
    a, b = open(plain).read().splitlines(), open(with_q).read().splitlines()
    assert a[0] + "\tlevel_q25\tlevel_median\tlevel_q75" == b[0] and len(a) == len(b) == 4
    assert [x.split("\t")[8:] for x in b[1:]] == [["-0.5", "0.125", "0.75"], ["-inf", "0.1", "inf"], ["1.0", "2.0", "3.0"]]
    assert [x.split("\t")[:8] for x in b] == [x.split("\t") for x in a]
    assert utils.SITE_QUANTILE_PROBS == (0.25, 0.5, 0.75)


# ---- dynamont-resquiggle --site-histogram ------------------------------------------------------------------------------------------
def test_cli_flag_and_its_parser():
    from dynamont_amd.segmentation import segment as seg
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).site_histogram == ""
    assert seg.parse(base + ["--site-summary", "s.tsv", "--site-histogram", "32:-4:4"]).site_histogram == "32:-4:4"
    assert utils.parse_site_histogram("32") == (32, None, None)
    assert utils.parse_site_histogram("32:-4:4") == (32, -4.0, 4.0)
    assert utils.parse_site_histogram("30:-3.3:4.1") == (30, -3.3, 4.1)
    for bad in ("", "x", "32:", "32:-4", "32:-4:4:5", "32:a:b", "3.5", "1", "255", "0", "32:4:-4", "32:4:4", "32:nan:4", "32:-inf:4"):
        with pytest.raises(ValueError, match="--site-histogram"):
            utils.parse_site_histogram(bad)
    mean, sd = np.array([-1.5, 0.2, 2.0]), np.array([0.1, 0.3, 0.2])
    assert utils.site_histogram_range(mean, sd) == (-1.5 - 4 * 0.3, 2.0 + 4 * 0.3)


def test_cli_refuses_the_flag_without_a_site_summary(models, tmp_path):
    """before anything is started: no aligner, no output file"""
    from dynamont_amd.segmentation import segment as seg
    out = str(tmp_path / "out.csv.zst")
    with pytest.raises(ValueError, match="--site-histogram counts beside the per-site table: it needs --site-summary FILE"):
        seg.segment(str(tmp_path), str(tmp_path / "m.bam"), 1, out, models["syn9"], "rna004", "basic", site_histogram="32:-4:4")
    with pytest.raises(ValueError, match="BINS must be 2 .. 254"):
        seg.segment(str(tmp_path), str(tmp_path / "m.bam"), 1, out, models["syn9"], "rna004", "basic", site_summary=str(tmp_path / "s.tsv"),
                    site_histogram="300")
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "s.tsv")
