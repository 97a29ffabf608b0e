"""CPU: the host half of the band-margin diagnostics (dyn_aligner_set_band_margin). The segment-end shortcut the kernel uses
equals the all-rows definition (tests/band_margin_cases.py) on the harness's cases and on 10 000 random staircases and paths;
three deliberately wrong readings of the definition each differ from it on those cases; the definition's band is the CPU
oracle's band; on the oracle's own paths the `*_squeezed_band50` reads touch a real band edge and a clean read at band 400 does
not; the reads of the GPU retry test are picked here, on the oracle alone; the new entry points exist and refuse what they
cannot serve."""
import os
import re
import subprocess

import numpy as np
import pytest

import band_margin_cases as bmc
import imperfect_families as fam
from conftest import ROOT
from dynamont_amd import Aligner, _native as N, synth
from dynamont_amd.segmentation import segment as seg
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("native_lib")


@pytest.fixture(scope="module")
def batch():
    return bmc.build_batch()


def test_harness_batch_holds_the_cases(batch):
    b = batch
    ref = bmc.reference(b)
    low, high, edge = ref
    labels = [r.label for r in b.reads]
    at = lambda s: next(i for i, lab in enumerate(labels) if lab.startswith(s))  # noqa: E731
    assert 20 <= len(b.reads) <= 60
    assert (b.read != np.arange(len(b.read))).sum() > len(b.read) // 2                 # processing order is not read order
    failed = np.flatnonzero(b.status != 0)
    assert len(failed) == 1 and 2 < failed[0] < 8 and tuple(ref[:, failed[0]]) == (bmc.NONE, bmc.NONE, 0)
    assert b.reads[0].N == 2 and {b.reads[2].N, b.reads[3].N} == {10, 11} and b.reads[2].bw == 5 and b.reads[3].bw == 5
    for s in ("N = 2", "T = N = 3", "a half band of N - 1"):                          # the band covers every column
        assert tuple(ref[:, at(s)]) == (bmc.NONE, bmc.NONE, 0), s
    i = at("only the upper edge")
    assert low[i] == bmc.NONE and high[i] != bmc.NONE
    i = at("only the lower edge")
    assert low[i] != bmc.NONE and high[i] == bmc.NONE
    i = at("on the lower edge for a run")
    assert low[i] == 0 and high[i] > 0 and edge[i] > 1000
    i = at("on the upper edge for a run")
    assert high[i] == 0 and low[i] > 0 and edge[i] > 1000
    i = at("bw = 1: a row on either")
    assert low[i] == 0 and high[i] == 0
    i = at("bw = 0")                                                                   # both slacks 0 on one row: counted once
    r = b.reads[i]
    both = sum(1 for t in range(int(r.segrow[0]), r.T) if bmc.mid(t, r.ratio) - r.bw >= 2 and bmc.mid(t, r.ratio) + r.bw + 1 < r.N)
    assert both > 50 and edge[i] == r.T - int(r.segrow[0]) - sum(
        1 for t in range(int(r.segrow[0]), r.T) if not (bmc.mid(t, r.ratio) >= 2 or bmc.mid(t, r.ratio) + 1 < r.N))
    assert {r.N - 1 for r in b.reads} >= {255, 256, 257, 1000}
    stalls = [max(np.diff(np.append(r.segrow.astype(np.int64), r.T))) for r in b.reads]
    assert sum(s >= 20001 for s in stalls) >= 1 and sum(s >= 19000 for s in stalls) >= 2
    i = at("a stall that lasts until")
    assert low[i] == 0 and edge[i] > 0
    i = at("a stall of 20 001 rows across")
    r = b.reads[i]
    j = int(np.argmax(np.diff(np.append(r.segrow.astype(np.int64), r.T))))
    assert bmc.mid(int(r.segrow[j + 1]) - 1, r.ratio) - bmc.mid(int(r.segrow[j]), r.ratio) > 100   # many staircase steps
    near = [r for r in b.reads if "within an ulp" in r.label]
    assert len(near) >= 4 and all(r.T > 99900 and bmc.near_integer_products(r.T, r.ratio).size for r in near)
    assert sum("T a multiple of N" in lab for lab in labels) == 2
    # the read range [2, 9) (a merged launch whose members did not all ask): the failed read inside, the rest untouched
    part = bmc.reference(b, 2, 9)
    assert (part[:, :2] == 0xdeadbeef).all() and (part[:, 9:] == 0xdeadbeef).all() and np.array_equal(part[:, 2:9], ref[:, 2:9])


def test_shortcut_equals_the_definition_on_the_cases(batch):
    assert np.array_equal(bmc.reference(batch, fn=bmc.shortcut), bmc.reference(batch))


def test_shortcut_equals_the_definition_on_random_staircases_and_paths():
    rng = np.random.default_rng(20261019)
    seen_none = seen_zero = seen_both = 0
    for k in range(10000):
        T = int(rng.integers(3, 160))
        N = int(rng.integers(2, T + 1))
        bw = min(int(rng.integers(1, 30)), N // 2)
        ratio = float(N) / float(T)
        segrow = bmc.make_path(T, N, bw, ratio, ("low", "high", "random")[k % 3], rng)
        want = bmc.brute(segrow, T, N, bw, ratio)
        assert bmc.shortcut(segrow, T, N, bw, ratio) == want, (T, N, bw, segrow.tolist())
        seen_none += want[0] == bmc.NONE or want[1] == bmc.NONE
        seen_zero += min(want[0], want[1]) == 0
        seen_both += want[0] != bmc.NONE and want[1] != bmc.NONE
    assert seen_none > 500 and seen_zero > 500 and seen_both > 500


@pytest.mark.parametrize("wrong", ["clamped", "ge1", "upper_last"])
def test_cases_tell_a_wrong_reading_apart(batch, wrong):
    """the edge counted as real where the lattice's border clamps it; mid - bw >= 1 instead of >= 2; the upper minimum taken on
    the segment's last row"""
    right = bmc.reference(batch)
    got = bmc.reference(batch, fn=bmc.shortcut, wrong=wrong)
    differs = np.flatnonzero((got != right).any(axis=0))
    assert differs.size >= 3, (wrong, differs)
    if wrong == "upper_last":
        assert np.array_equal(got[0], right[0]) and not np.array_equal(got[1], right[1])


def test_the_definitions_band_is_the_oracles(models):
    """nStart / nEnd of the oracle's computeBounds: the lower edge is real iff nStart >= 2 (a column of 1 .. N-1 is excluded), the
    upper iff nEnd < N; the slacks are the distances to nStart and nEnd - 1"""
    orc = Oracle(models["syn5"], 0)
    for T, N, band in [(90, 10, 50), (300, 40, 50), (1027, 256, 50), (400, 36, 36), (120, 30, 2), (2000, 333, 400)]:
        bw = min(band // 2, N // 2)
        ratio = float(N) / float(T)
        _, n_start, n_end = orc.bounds(T, N, bw)
        for t in range(1, T):
            m = bmc.mid(t, ratio)
            assert (m - bw >= 2) == (int(n_start[t]) >= 2) and (m + bw + 1 < N) == (int(n_end[t]) < N)
            if m - bw >= 2:
                assert m - bw == int(n_start[t])
            if m + bw + 1 < N:
                assert m + bw == int(n_end[t]) - 1


def oracle_margins(orc, read, band):
    res = orc.align(read.signal, read.sequence, True)
    ns = len(res["signal_positions"])
    T, Ncols = len(read.signal) + 1, ns + 1
    segrow = res["signal_positions"].astype(np.int64) + 1                              # signal position = lattice row - 1
    return bmc.brute(segrow, T, Ncols, min(band // 2, Ncols // 2), float(Ncols) / float(T))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    return fam.write_tables(str(tmp_path_factory.mktemp("bm_tables")), ["syn5", "syn9"])


@pytest.mark.parametrize("pore", ["rna002", "dna_r10_400bps"])
def test_squeezed_reads_touch_a_real_edge_on_the_oracle(tables, pore):
    name = pore + "_squeezed_band50"
    f = fam.FAMILIES[name]
    orc = Oracle(tables[f.table][0], synth.PORES[pore][0], f.band)
    touched = 0
    for r in fam.reads_of(name, tables):
        low, high, edge = oracle_margins(orc, r, f.band)
        if min(low, high) == 0:
            assert edge > 0
            touched += 1
        else:
            assert edge == 0
    assert touched >= fam.N_READS // 2                                                 # "the path leaves the band"


def test_a_clean_read_at_band_400_keeps_its_distance(models):
    _, mean, sd = synth.read_model_file(models["syn5"])
    orc = Oracle(models["syn5"], 0, 400)
    for r in synth.make_reads(7101, 3, "rna002", mean, sd, (500, 700)):               # N > 401: both edges are real somewhere
        low, high, edge = oracle_margins(orc, r, 400)
        assert low != bmc.NONE and high != bmc.NONE and min(low, high) > 0 and edge == 0


def test_the_retry_reads_are_picked_on_the_oracle_alone(tables):
    """every flagged read shows a margin below RETRY_MIN_MARGIN at band 50 and reaches it at the band recorded, the first of the
    chain that does; every clean read passes at band 50"""
    f = fam.FAMILIES[bmc.RETRY_FAMILY]
    assert f.band == bmc.RETRY_CHAIN[0] == 50
    reads = fam.reads_of(bmc.RETRY_FAMILY, tables)
    orcs = {band: Oracle(tables[f.table][0], synth.PORES[f.pore][0], band) for band in bmc.RETRY_CHAIN}
    for i, first_ok in bmc.RETRY_FLAGGED.items():
        for band in bmc.RETRY_CHAIN:
            low, high, _ = oracle_margins(orcs[band], reads[i], band)
            assert (min(low, high) >= bmc.RETRY_MIN_MARGIN) == (band == first_ok), (i, band, low, high)
            if band == first_ok:
                break
    assert set(bmc.RETRY_FLAGGED.values()) == {100, 200}                               # one retry and two
    for i in bmc.RETRY_CLEAN:
        low, high, _ = oracle_margins(orcs[50], reads[i], 50)
        assert min(low, high) >= bmc.RETRY_MIN_MARGIN


def test_the_new_symbols(native_lib, models):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_band_margin", "dyn_batch_fetch_band_margin"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "DYN_BAND_MARGIN_NONE 0xFFFFFFFFu" in hdr and N.DYN_BAND_MARGIN_NONE == bmc.NONE
    assert re.search(r"typedef struct dyn_band_margin_out \{\s*uint32_t\* low;[^}]*uint32_t\* high;[^}]*uint32_t\* edge_rows;[^}]*uint64_t n;", hdr)


def test_entry_points_refuse_what_they_cannot_serve(native_lib, models):
    assert native_lib.dyn_aligner_set_band_margin(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_batch_fetch_band_margin(None, None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")          # no device: as every entry point that needs one
    for on in (True, False):
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            al.set_band_margin(on)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.set_band_retry(1)
    al.set_band_retry(0)                                           # off: nothing to refuse
    with pytest.raises(ValueError):
        al.set_band_retry(1, factor=1)
    al.close()
    ntk = Aligner(models["syn9"], "rna004", mode="resquiggle", device="host")
    with pytest.raises(ValueError, match="modes ntk / resquiggle"):
        ntk.set_band_margin(True)
    ntk.close()


def test_cli_flag():
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).band_report == ""
    assert seg.parse(base + ["--band-report", "out.tsv"]).band_report == "out.tsv"


def test_band_report_lines():
    lines = seg.band_report_lines(["b", "a"], [101, 51], [11, 6], 400, np.array([bmc.NONE, 3], dtype=np.uint32),
                                  np.array([0, bmc.NONE], dtype=np.uint32), np.array([7, 0], dtype=np.uint32))
    assert lines == ["b\t101\t11\t400\t\t0\t7", "a\t51\t6\t400\t3\t\t0"]
    assert seg.band_report_bytes(lines) == (b"readid\tT\tN\tband\tband_margin_low\tband_margin_high\tband_edge_rows\n"
                                             b"a\t51\t6\t400\t3\t\t0\nb\t101\t11\t400\t\t0\t7\n")


def test_kernels_compile_with_the_products_flags_without_scratch_or_lds(tmp_path):
    """tests/device_math/band_margin.hip builds with the product's flags; the compiler's resource remarks show two kernels
    without scratch and without LDS, well inside the 152 VGPRs a resident workgroup leaves"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "band_margin.hip"), "-o", str(tmp_path / "libbm.so")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert scratch == [0, 0] and lds == [0, 0] and len(vgprs) == 2 and max(vgprs) <= 64, (scratch, lds, vgprs)
