"""CPU: the host half of the sparse per-site table (dyn_aligner_set_site_summary_sparse). The header text and the symbols; what a
handle without a device refuses; the footprint of every kernel of tests/device_math/site_map.hip as the compiler reports it; the
map header without kernels; the restatement of tests/site_map_cases.py against the dense cases' references and against a plain
model of the map."""
import os
import re
import subprocess

import numpy as np
import pytest

import site_histogram_cases as shc
import site_map_cases as smc
import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native as N

pytestmark = pytest.mark.usefixtures("native_lib")

SYMBOLS = ("dyn_aligner_set_site_summary_sparse", "dyn_aligner_site_map_stats", "dyn_aligner_site_map_keys", "dyn_aligner_site_map_windows")


def test_header_text_and_symbols(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION (\d+)\b", hdr).group(1) == "10"        # added within ABI 10
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    flat = " ".join(hdr.split())
    assert "int dyn_aligner_set_site_summary_sparse(dyn_aligner* a, uint64_t num_sites, uint64_t capacity);" in flat
    assert "int dyn_aligner_site_map_stats(dyn_aligner* a, uint64_t out[4]);" in flat
    assert "int dyn_aligner_site_map_keys(dyn_aligner* a, uint64_t bucket_lo, uint64_t bucket_hi, uint32_t* keys);" in flat
    assert "int dyn_aligner_site_map_windows(dyn_aligner* a, int shift, uint64_t* windows, uint64_t cap, uint64_t* count);" in flat
    assert "site_map.hpp" in N.HEADERS and "site_map_kernels.hpp" in N.HEADERS


def test_entry_points_refuse_what_they_cannot_serve(native_lib, models):
    assert native_lib.dyn_aligner_set_site_summary_sparse(None, 5, 5) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_map_stats(None, None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_map_keys(None, 0, 0, None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_map_windows(None, 20, None, 0, None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")
    assert native_lib.dyn_aligner_set_site_summary_sparse(al._h, 100, 10) == N.DYN_ERR_DEVICE
    with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
        al.set_site_summary(smc.ID_SPACE, capacity=4096)
    with pytest.raises(ValueError, match="not below DYN_SITE_NONE"):
        al.set_site_summary(0xFFFFFFFF, capacity=4096)
    with pytest.raises(ValueError, match="capacity 4294967295 is not below 4294967295"):
        al.set_site_summary(100, capacity=0xFFFFFFFF)
    with pytest.raises(ValueError, match="capacity must be None"):
        al.set_site_summary(100, capacity=0)
    assert native_lib.dyn_aligner_set_site_summary_sparse(al._h, 100, 0) == N.DYN_ERR_INVALID_ARGUMENT
    assert "capacity 0 is no table" in al.last_error()
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_map()
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_map_keys(0, 0)
    with pytest.raises(ValueError, match="shift 32 is not 0 .. 31"):
        al.site_map_windows(32)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_map_windows()
    al._band_retry = (2, 4093, 2)
    with pytest.raises(ValueError, match="set_site_summary with set_band_retry"):
        al.set_site_summary(10, capacity=10)
    al.close()
    ntk = Aligner(models["syn9"], "rna004", mode="resquiggle", device="host")
    with pytest.raises(ValueError, match="modes ntk / resquiggle"):
        ntk.set_site_summary(10, capacity=10)
    ntk.close()
    with pytest.raises(NotImplementedError, match="MultiAligner has no per-site summary"):
        MultiAligner.set_site_summary(None, 10, capacity=10)


def test_kernels_compile_with_the_products_flags_beside_a_resident_workgroup(tmp_path):
    """tests/device_math/site_map.hip builds for gfx950 with the product's flags; the compiler's resource remarks show the two
    filling kernels (now with the probe loop) and the three window kernels without scratch, within 13 KB of static LDS and 152
    VGPRs"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "site_map.hip"), "-o", str(tmp_path / "libsm.so")]
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(x) for x in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    vgprs = [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)]
    assert len(names) == 5
    for k in ("k_ssum_short", "k_ssum_long", "k_site_gather", "k_site_scatter_add", "k_site_map_windows"):
        assert any(k in n for n in names), (k, names)
    print(dict(zip(names, zip(scratch, lds, vgprs))))
    assert scratch == [0] * 5 and max(lds) <= 13 * 1024 and max(vgprs) <= 152, (scratch, lds, vgprs)


def test_the_map_header_has_no_kernels_and_the_window_kernels_one_unit():
    src = lambda f: open(os.path.join(N.CSRC, f)).read()  # noqa: E731
    assert "__global__" not in src("site_map.hpp")
    assert len(re.findall(r"__global__", src("site_summary_kernels.hpp"))) == 2      # k_ssum_short, k_ssum_long and no third one
    assert len(re.findall(r"__global__", src("site_map_kernels.hpp"))) == 3
    users = [f for f in os.listdir(N.CSRC) if '#include "site_map_kernels.hpp"' in src(f)]
    assert users == ["site_summary.hip"]


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def model_home(ids, capacity):
    """a stand-in hash for the host tests (the device tests take the real one from the harness)"""
    return (np.asarray(ids, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 32) * np.uint64(capacity) >> np.uint64(32)).astype(np.uint32)


def model_insert(keys, k, home, probe_max=smc.PROBE_MAX):
    cap = len(keys)
    h = int(home([k], cap)[0])
    for _ in range(min(cap, probe_max)):
        if keys[h] in (smc.EMPTY, k):
            keys[h] = k
            return h
        h = (h + 1) % cap
    return None


def test_dict_restatement_equals_the_dense_cases():
    """the ids of the dense cases sent through scatter_ids: the dict restatement holds, per id, what the list restatement holds
    per site -- table, totals and both histograms"""
    table = smc.scatter_ids()
    assert len(set(table[s] for s in range(ssc.NUM_SITES))) == ssc.NUM_SITES and max(table[s] for s in range(ssc.NUM_SITES)) < smc.ID_SPACE
    assert sum(table[s] >= 4000000000 for s in range(ssc.NUM_SITES)) >= ssc.NUM_SITES // 2 and table[ssc.NUM_SITES] == smc.ID_SPACE
    b0 = shc.build_batch()
    reads = smc.remap(b0.reads, table)
    hist = {}
    want, dropped = smc.reference(reads, hist=hist, spec=shc.ROUNDED)
    dense, dense_h = ssc.reference(b0), shc.reference(b0, *shc.ROUNDED)
    assert dropped == 0 and want["totals"] == dense["totals"]
    for s in range(ssc.NUM_SITES):
        c = want["cells"].get(table[s], [0] * 5)
        assert c == [dense[f][s] for f in smc.FIELDS], s
        lv, dw = hist.get(table[s], ([0] * (shc.ROUNDED[0] + 2), [0] * 16))
        assert lv == dense_h["level"][s] and dw == dense_h["dwell"][s], s
    assert set(want["cells"]) <= set(table.values())
    # limbs and back
    for c in want["cells"].values():
        assert smc.from_limbs(smc.cell_limbs(c)) == [c[0], c[1], c[2] & ssc.M64, c[3], c[4]]
    b = smc.pack(reads)
    assert b.num_sites == smc.ID_SPACE and b.sites.dtype == np.uint32 and int(b.sites.max()) == smc.EMPTY


def test_dropped_rows_are_whole_keys_and_the_totals_account_for_every_row():
    keys = [7, 8, 9, 4000000000]
    reads = smc.contended_reads(keys, 3, 4, seed=1, long_rows=((3, 300),))
    rows = sum(len(segs) for _, segs in reads)
    full, d0 = smc.reference(reads)
    part, d1 = smc.reference(reads, present={7, 4000000000})
    assert d0 == 0 and d1 == 2 * 12 and set(part["cells"]) == {7, 4000000000}
    assert all(part["cells"][k] == full["cells"][k] for k in part["cells"])          # a present key's cell is complete
    t = part["totals"]
    assert t["rows_added"] + t["rows_without_site"] + t["rows_skipped"] == rows and t["rows_skipped"] == d1
    assert full["cells"][4000000000][0] == 13 and min(len(segs) for _, segs in reads[:3]) == 16


def test_check_map_tells_a_broken_map_apart():
    """a model map filled by linear probing passes; a duplicated key, a key beyond its probe window, a hole before a key, a stale
    cell and a wrong n_keys are each refused"""
    cap = 64
    home = lambda ids: model_home(ids, cap)  # noqa: E731
    ids = smc.same_home_ids(model_home, cap, 60, 10, limit=1 << 16)             # wraps: buckets 60 .. 63, 0 .. 5
    keys = np.full(cap, smc.EMPTY, dtype=np.uint32)
    rows = [model_insert(keys, k, model_home) for k in ids]
    assert rows == [(60 + i) % cap for i in range(10)]
    cells = np.zeros((cap, 7), dtype=np.uint64)
    cells[rows, 0] = 1
    assert smc.check_map(keys, cells, 10, home) == dict(zip(ids, rows))
    assert smc.check_map(keys, cells, 10, home, probe_max=10) == dict(zip(ids, rows))
    with pytest.raises(AssertionError):
        smc.check_map(keys, cells, 9, home)
    with pytest.raises(AssertionError, match="probe window"):
        smc.check_map(keys, cells, 10, home, probe_max=9)
    bad = keys.copy()
    bad[20] = ids[0]
    with pytest.raises(AssertionError, match="two buckets"):
        smc.check_map(bad, cells, 11, home)
    bad = keys.copy()
    bad[62] = smc.EMPTY
    c2 = cells.copy()
    c2[62] = 0
    with pytest.raises(AssertionError, match="empty bucket before"):
        smc.check_map(bad, c2, 9, home)
    with pytest.raises(AssertionError, match="not zero"):
        smc.check_map(bad, cells, 9, home)
    # a full map of 8 rows takes 8 keys of 20 and no more
    small = np.full(8, smc.EMPTY, dtype=np.uint32)
    got = [model_insert(small, k, model_home) for k in range(100, 120)]
    assert sum(r is not None for r in got) == 8 and (small != smc.EMPTY).all()


# ---- dynamont-resquiggle --site-capacity: the flag, its refusals, the walk over the occupied windows ---------------------------
def test_cli_flag_and_its_refusals(models, tmp_path):
    """refused before anything is started: no aligner, no output file"""
    from dynamont_amd import bam_io
    from dynamont_amd.segmentation import segment as seg
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).site_capacity == 0
    assert seg.parse(base + ["--site-summary", "s.tsv", "--site-capacity", "4096"]).site_capacity == 4096
    tags = dict(qs=12.5, ns=5000, ts=10, fn="reads.pod5", sm=90.0, sd=15.0)
    mapped = str(tmp_path / "m.bam")
    bam_io.write_bam(mapped, [("r0", "ACGTACGTACGT", dict(tags), (0, 0, 3, [12 << 4]))], references=[("chrA", 100)])
    out = str(tmp_path / "out.csv.zst")
    args = (str(tmp_path), mapped, 1, out, models["syn9"], "rna004", "basic")
    with pytest.raises(ValueError, match="--site-capacity sizes the sparse per-site table: it needs --site-summary FILE"):
        seg.segment(*args, site_capacity=100)
    for rows in (-5, 4294967295):
        with pytest.raises(ValueError, match="ROWS must be 1 .. 4294967294"):
            seg.segment(*args, site_summary=str(tmp_path / "s.tsv"), site_capacity=rows)
    assert not os.path.exists(out) and not os.path.exists(tmp_path / "s.tsv")


def test_writers_walk_only_the_listed_windows_and_write_the_same_lines(tmp_path):
    from dynamont_amd._dynamont import site_summary_from_limbs
    from dynamont_amd.segmentation.utils import load_site_table, save_site_table, write_site_summary
    from dynamont_amd.sites import contig_offsets
    n = 40
    acc = ssc.empty(n)
    for s, v in {1: 2, 5: 1, 17: 3, 18: 1, 39: 4}.items():               # windows of 4 sites: 0, 1, 4 and 9 hold a site
        acc["n_rows"][s], acc["n_samples"][s], acc["dwell_sq"][s], acc["M1"][s], acc["M2"][s] = v, 10 * v, 100 * v, v << 40, v << 41
    full = site_summary_from_limbs(*ssc.limbs(acc))
    calls = []

    def fetch(lo, hi):                                               # what Aligner.site_summary(lo, hi) returns
        calls.append((lo, hi))
        return {k: (v[lo:hi] if k not in ("limbs", "totals") else ([c[lo:hi] for c in v] if k == "limbs" else v)) for k, v in full.items()}

    refs, offs = ["chrA", "chrB"], contig_offsets([25, 15])
    dense, sparse = str(tmp_path / "d.tsv"), str(tmp_path / "s.tsv")
    assert write_site_summary(dense, fetch, n, refs, offs, window=4) == 5 and len(calls) == 10
    del calls[:]
    assert write_site_summary(sparse, fetch, n, refs, offs, window=4, windows=[9, 0, 4, 1, 12]) == 5   # any order; 12 lies outside
    assert calls == [(0, 4), (4, 8), (16, 20), (36, 40)]
    assert open(sparse).read() == open(dense).read()
    del calls[:]
    assert write_site_summary(sparse, fetch, n, refs, offs, window=4, windows=[]) == 0 and calls == []
    assert open(sparse).read() == open(dense).readline()             # the header alone

    class Handle:                                                    # what save_site_table asks of an Aligner
        _site_histogram = None
        site_summary = staticmethod(fetch)

    del calls[:]
    assert save_site_table(str(tmp_path / "d.npz"), Handle, refs, [25, 15], window=4) == 5 and len(calls) == 10
    del calls[:]
    assert save_site_table(str(tmp_path / "s.npz"), Handle, refs, [25, 15], window=4, windows=[0, 1, 4, 9]) == 5
    assert calls == [(0, 4), (4, 8), (16, 20), (36, 40)]
    a, b = load_site_table(str(tmp_path / "d.npz")), load_site_table(str(tmp_path / "s.npz"))
    assert a["site"].tolist() == b["site"].tolist() == [1, 5, 17, 18, 39]
    assert all(np.array_equal(x, y) for x, y in zip(a["limbs"], b["limbs"]))
    # a window [lo, hi) that does not start on a window border: the listed windows are cut to it
    del calls[:]
    assert save_site_table(str(tmp_path / "c.npz"), Handle, refs, [25, 15], lo=5, hi=38, window=4, windows=[0, 1, 4, 9]) == 3
    assert calls == [(5, 8), (16, 20), (36, 38)] and load_site_table(str(tmp_path / "c.npz"))["site"].tolist() == [0, 12, 13]
