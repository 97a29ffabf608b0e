"""CPU: the host half of the per-site table by content (dyn_aligner_site_pack, dyn_aligner_site_summary_merge). The header text
and the symbols; what a handle without a device refuses, argument refusals first; the footprint of the four kernels of
tests/device_math/site_pack.hip as the compiler reports it; the restatement of tests/site_pack_cases.py on tables small enough to
check by eye; dynamont-resquiggle's --site-merge-ranks and --site-table-in: the flags, their refusals, the old refusal unchanged."""
import os
import re
import subprocess

import numpy as np
import pytest

import site_pack_cases as spc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native as N

pytestmark = pytest.mark.usefixtures("native_lib")

SYMBOLS = ("dyn_aligner_site_pack", "dyn_aligner_site_summary_merge")
KERNELS = ("k_site_pack_count", "k_site_pack_scan", "k_site_pack_write", "k_site_merge")


def test_header_text_and_symbols(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION (\d+)\b", hdr).group(1) == "10"        # added within ABI 10
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    flat = " ".join(hdr.split())
    assert "int dyn_aligner_site_pack(dyn_aligner* a, uint64_t row_lo, uint64_t row_hi, uint64_t site_lo, uint64_t site_hi, uint64_t cap," in flat
    assert "int dyn_aligner_site_summary_merge(dyn_aligner* a, uint64_t count, const uint32_t* site, uint64_t offset, const uint64_t* cells," in flat
    assert "site_pack_kernels.hpp" in N.HEADERS
    assert len(N.SIGNATURES["dyn_aligner_site_pack"][1]) == 11 and len(N.SIGNATURES["dyn_aligner_site_summary_merge"][1]) == 8


def test_kernels_live_in_one_header_and_one_unit():
    src = lambda f: open(os.path.join(N.CSRC, f)).read()  # noqa: E731
    text = src("site_pack_kernels.hpp")
    assert re.findall(r"__global__ __launch_bounds__\(256\) void (\w+)", text) == list(KERNELS)
    users = [f for f in os.listdir(N.CSRC) if '#include "site_pack_kernels.hpp"' in src(f)]
    assert users == ["site_summary.hip"]
    merge = text.split("void k_site_merge")[1]
    assert "sm_find_or_insert" in merge and "xs_add128(cell + 3" in merge and "xs_add128(cell + 5" in merge and "SM_SITES_DROPPED" in merge
    pack = text.split("void k_site_merge")[0]
    assert "atomic" not in pack.split("namespace dynk")[1].replace("__hip_atomic_load", "")   # no cursor: count, scan, write
    assert "smk_load64" in pack and "smk_load32" in pack and "__ballot" in pack
    # the kernels beside them keep their place
    assert len(re.findall(r"__global__", src("site_map_kernels.hpp"))) == 3


def test_entry_points_refuse_what_they_cannot_serve(native_lib, models):
    u32 = np.zeros(64, dtype=np.uint32)
    u64 = np.zeros(64, dtype=np.uint64)
    p32, p64 = u32.ctypes.data_as(N.c_u32_p), u64.ctypes.data_as(N.c_u64_p)
    assert native_lib.dyn_aligner_site_pack(None, 0, 1, 0, 1, 1, p32, p64, None, None, p64) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_summary_merge(None, 1, p32, 0, p64, None, None, None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")
    # argument refusals come before the device is looked at: the same text on a handle without one
    assert native_lib.dyn_aligner_site_pack(al._h, 0, 1, 0, 1, 1, p32, p64, None, None, None) == N.DYN_ERR_INVALID_ARGUMENT    # no count
    assert native_lib.dyn_aligner_site_pack(al._h, 0, 1, 0, 1, 1, None, p64, None, None, p64) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_pack(al._h, 0, 1, 0, 1, 1, p32, p64, p32, None, p64) == N.DYN_ERR_INVALID_ARGUMENT
    assert al.last_error() == "dyn_aligner_site_pack: level and dwell counters are given together or not at all"
    assert native_lib.dyn_aligner_site_summary_merge(al._h, 1, p32, 0, p64, None, None, p32) == N.DYN_ERR_INVALID_ARGUMENT
    assert al.last_error() == "dyn_aligner_site_summary_merge: level and dwell counters are given together or not at all"
    assert native_lib.dyn_aligner_site_summary_merge(al._h, 1, None, 0, p64, None, None, None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_pack(al._h, 2, 1, 0, 1, 1, p32, p64, None, None, p64) == N.DYN_ERR_INVALID_ARGUMENT
    assert al.last_error() == "dyn_aligner_site_pack: [2, 1) is not a range of rows"
    assert native_lib.dyn_aligner_site_pack(al._h, 0, 1, 9, 3, 1, p32, p64, None, None, p64) == N.DYN_ERR_INVALID_ARGUMENT
    assert al.last_error() == "dyn_aligner_site_pack: [9, 3) is not a range of sites"
    # an empty range of rows or of ids is DYN_OK with count 0 and touches nothing, the device included
    u64[0] = 77
    assert native_lib.dyn_aligner_site_pack(al._h, 5, 5, 0, 1, 0, None, None, None, None, p64) == N.DYN_OK and u64[0] == 0
    u64[0] = 77
    assert native_lib.dyn_aligner_site_pack(al._h, 0, 10, 4, 4, 1, p32, p64, None, None, p64) == N.DYN_OK and u64[0] == 0
    assert native_lib.dyn_aligner_site_summary_merge(al._h, 0, None, 0, None, None, None, None) == N.DYN_ERR_DEVICE   # (the conditions of the fetch)
    # ... and what is left needs the device
    assert native_lib.dyn_aligner_site_pack(al._h, 0, 1, 0, 1, 1, p32, p64, None, None, p64) == N.DYN_ERR_DEVICE
    assert native_lib.dyn_aligner_site_summary_merge(al._h, 1, p32, 0, p64, None, None, None) == N.DYN_ERR_DEVICE
    al._site_table = 100
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_table_pack()
    packed = {"site": np.arange(3, dtype=np.uint64), "limbs": [np.ones(3, dtype=np.uint64)] * 7, "totals": [1, 2, 3, 4, 5]}
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_summary_merge(packed)
    # the Python checks, before the call
    with pytest.raises(ValueError, match="seven columns of one entry per site"):
        al.site_summary_merge(dict(packed, limbs=[np.ones(3, dtype=np.uint64)] * 6 + [np.ones(2, dtype=np.uint64)]))
    with pytest.raises(ValueError, match="five totals"):
        al.site_summary_merge(dict(packed, totals=[1, 2]))
    with pytest.raises(ValueError, match="offset must be >= 0"):
        al.site_summary_merge(packed, offset=-1)
    with pytest.raises(ValueError, match="integer ids below 4294967295"):
        al.site_summary_merge(dict(packed, site=np.array([0, 1, 0xFFFFFFFF], dtype=np.uint64)))
    with pytest.raises(ValueError, match="level and dwell counters are given together or not at all"):
        al.site_summary_merge(dict(packed, level=np.zeros((3, 7), dtype=np.uint32)))
    al._site_histogram = (5, -1.0, 1.0)
    mine = -1.0 + np.arange(6, dtype=np.float64) * (2.0 / 5)
    hist = dict(level=np.zeros((3, 7), dtype=np.uint32), dwell=np.zeros((3, 16), dtype=np.uint32))
    with pytest.raises(ValueError, match=r"the histogram's edges are not the handle's \(set_site_histogram\(5, -1.0, 1.0\)\)"):
        al.site_summary_merge(dict(packed, edges=np.nextafter(mine, 2.0), **hist))
    with pytest.raises(ValueError, match=r"level must be \[n, bins \+ 2\] and dwell \[n, 16\]"):
        al.site_summary_merge(dict(packed, edges=mine, level=np.zeros((3, 8), dtype=np.uint32), dwell=hist["dwell"]))
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_summary_merge(dict(packed, edges=mine, **hist))
    al.close()
    for call in (lambda: MultiAligner.site_table_pack(None), lambda: MultiAligner.site_summary_merge(None, packed)):
        with pytest.raises(NotImplementedError, match="MultiAligner has no per-site summary .*use one Aligner per device"):
            call()


def test_kernels_compile_with_the_products_flags_beside_a_resident_workgroup(tmp_path):
    """tests/device_math/site_pack.hip builds for gfx950 with the product's flags; the compiler's resource remarks show the three
    passes of the pack and the merge without scratch, within 13 KB of static LDS and 152 VGPRs"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "site_pack.hip"), "-o", str(tmp_path / "libsp.so")]
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S)
    vgprs = dict(re.findall(r"Function Name: (\S+).*? VGPRs: (\d+)", r.stderr, re.S))
    seen = {}
    for k in KERNELS:
        hit = [(n, int(s), int(l)) for n, s, l in blocks if k in n]
        assert len(hit) == 1, (k, [n for n, _, _ in blocks])
        seen[k] = (hit[0][1], hit[0][2], int(vgprs[hit[0][0]]))
    print(seen)
    for k, (scratch, lds, v) in seen.items():
        assert scratch == 0 and lds <= 13 * 1024 and v <= 152, (k, scratch, lds, v)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_pack_restatement_by_hand():
    cells = np.zeros((6, 7), dtype=np.uint64)
    hist = np.zeros((6, 23), dtype=np.uint32)
    cells[1, 6] = 9                      # only m2_hi
    hist[3, 22] = 4                      # only the last dwell counter
    cells[4] = 1
    dense = spc.pack_reference(None, cells, hist, 0, 6, 0, 6)
    assert [r[0] for r in dense] == [1, 3, 4] and dense[0][1] == [0, 0, 0, 0, 0, 0, 9] and dense[1][2][22] == 4 and not any(dense[1][1])
    assert [r[0] for r in spc.pack_reference(None, cells, hist, 2, 3, 0, 6)] == [3, 4]
    assert [r[0] for r in spc.pack_reference(None, cells, hist, 0, 6, 0, 4)] == [1, 3]                 # the filter's end is open
    assert [r[0] for r in spc.pack_reference(None, cells, None, 0, 6, 0, 6)] == [1, 4]                 # the table alone
    keys = np.array([50, spc.EMPTY, 7, 30, 40, 60], dtype=np.uint32)                                   # bucket order, not id order
    sparse = spc.pack_reference(keys, cells, hist, 0, 6, 0, 100)
    assert [r[0] for r in sparse] == [30, 40]        # bucket 1 is empty, buckets 0, 2 and 5 hold a key and all-zero words
    assert [r[0] for r in spc.pack_reference(keys, cells, hist, 0, 6, 0, 40)] == [30]                  # a key equal to site_hi is outside
    site, c, h = spc.records_as_arrays(sparse, 23)
    assert site.dtype == np.uint32 and c.shape == (2, 7) and h.shape == (2, 23)
    assert spc.records_as_arrays([], 23)[2].shape == (0, 23)


def test_merge_restatement_by_hand():
    M64 = spc.M64
    table = {}
    rec = (5, [1, 2, 3, M64, 0, M64, M64], [0xFFFFFFFF, 1])
    assert spc.merge_reference(table, [rec, rec], offset=10) == 0
    w, c = table[15]
    assert w == [2, 4, 6, M64 - 1, 1, M64 - 1, M64] and c == [0xFFFFFFFE, 2]     # the carry reaches m1_hi; -1 twice is -2; the counter wraps
    assert spc.merge_reference(table, [(9, [0] * 7, [0, 0])]) == 0 and 9 not in table                  # an all-zero record takes no row
    assert spc.merge_reference(table, [(1, [1] + [0] * 6, [0, 0]), (2, [0] * 7, [0, 1]), (15, [1] * 7, [0, 0])], present={15, 2}) == 1
    assert 1 not in table and table[2][1] == [0, 1] and table[15][0][0] == 3
    t2 = {}
    spc.merge_reference(t2, [(0, [M64, 0, 0, 0, 0, 0, 0], [])] * 2)
    assert t2[0][0][0] == M64 - 1                                                                      # n_rows is mod 2^64


def test_live_patterns():
    for rows in (0, 1, 16, 17):
        assert spc.live_pattern("none", rows).sum() == 0 and spc.live_pattern("all", rows).sum() == rows
        assert spc.live_pattern("alternating", rows).sum() == (rows + 1) // 2 and spc.live_pattern("last", rows).sum() == min(rows, 1)
    rng = np.random.default_rng(1)
    cells, hist = spc.random_rows(rng, 17, 23, spc.live_pattern("alternating", 17))
    assert (cells[::2] != 0).all() and not cells[1::2].any() and (hist[::2] != 0).all() and not hist[1::2].any()
    assert spc.width(5) == 23 and spc.width(0) == 0 and spc.SCAN_TILE_ROWS % spc.CHUNK_ROWS == 0


# ---- dynamont-resquiggle --site-merge-ranks / --site-table-in: the flags, their refusals ----------------------------------------------
def test_cli_flags():
    from dynamont_amd.segmentation import segment as seg
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    a = seg.parse(base)
    assert a.site_merge_ranks is False and a.site_table_in == []
    a = seg.parse(base + ["--site-summary", "s.tsv", "--site-merge-ranks", "--site-table-in", "a.npz", "--site-table-in", "b.npz"])
    assert a.site_merge_ranks is True and a.site_table_in == ["a.npz", "b.npz"]


def test_cli_refusals(models, tmp_path, monkeypatch):
    """all before anything is started: no aligner, no process group, no output file"""
    from dynamont_amd import bam_io
    from dynamont_amd.segmentation import segment as seg
    from dynamont_amd.segmentation import utils as U
    tags = dict(qs=12.5, ns=5000, ts=10, fn="reads.pod5", sm=90.0, sd=15.0)
    ubam, mapped = str(tmp_path / "u.bam"), str(tmp_path / "m.bam")
    bam_io.write_bam(ubam, [("r0", "ACGTACGTACGT", dict(tags))])
    bam_io.write_bam(mapped, [("r0", "ACGTACGTACGT", dict(tags), (0, 0, 3, [12 << 4]))], references=[("chrA", 100)])
    out, tsv = str(tmp_path / "out.csv.zst"), str(tmp_path / "s.tsv")
    args = (str(tmp_path), mapped, 1, out, models["syn9"], "rna004", "basic")
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="--site-merge-ranks adds the ranks' per-site tables: it needs --site-summary FILE"):
        seg.segment(*args, site_merge_ranks=True)
    with pytest.raises(ValueError, match="--site-table-in adds a saved per-site table into the run's: it needs --site-summary FILE"):
        seg.segment(*args, site_table_in=("t.npz",))
    monkeypatch.setenv("WORLD_SIZE", "2")
    # without the flag the refusal keeps its text, and names the flag behind it
    with pytest.raises(ValueError, match="--site-summary runs in one process: merging the per-site tables of several ranks is not built yet") as e:
        seg.segment(*args, site_summary=tsv)
    assert "--site-merge-ranks" in str(e.value)
    # with the flag the run gets past it, to the next refusal
    with pytest.raises(ValueError, match="has no reference sequences"):
        seg.segment(str(tmp_path), ubam, 1, out, models["syn9"], "rna004", "basic", site_summary=tsv, site_merge_ranks=True)
    monkeypatch.delenv("WORLD_SIZE")
    # --site-table-in: a file of other references, one without histograms in a run with them, other bins
    def table(path, names, lengths, spec):
        class Fake:
            _site_histogram = spec
            def site_summary(self, lo, hi):
                z = np.zeros(hi - lo, dtype=np.uint64)
                return {"n_rows": z, "limbs": [z] * 7, "totals": dict.fromkeys(("reads_ok", "rows_added", "samples_added", "rows_without_site", "rows_skipped"), 0)}
            def site_histogram(self, lo, hi):
                return {"level": np.zeros((hi - lo, spec[0] + 2), dtype=np.uint32), "dwell": np.zeros((hi - lo, 16), dtype=np.uint32)}
        U.save_site_table(path, Fake(), names, lengths)
        return path
    other = table(str(tmp_path / "other.npz"), ["chrB"], [100], None)
    longer = table(str(tmp_path / "longer.npz"), ["chrA"], [101], None)
    plain = table(str(tmp_path / "plain.npz"), ["chrA"], [100], None)
    bins8 = table(str(tmp_path / "bins8.npz"), ["chrA"], [100], (8, -4.0, 4.0))
    with pytest.raises(ValueError, match="--site-table-in .*other.npz: its reference names differ from the BAM header's"):
        seg.segment(*args, site_summary=tsv, site_table_in=(plain, other))
    with pytest.raises(ValueError, match="--site-table-in .*longer.npz: its reference lengths differ"):
        seg.segment(*args, site_summary=tsv, site_table_in=(longer,))
    with pytest.raises(ValueError, match="--site-table-in .*plain.npz: the file holds no histograms"):
        seg.segment(*args, site_summary=tsv, site_histogram="32:-4:4", site_table_in=(plain,))
    with pytest.raises(ValueError, match=r"--site-table-in .*bins8.npz: its histograms \(8 bins over \[-4.0, 4.0\)\) are not the run's \(32 bins"):
        seg.segment(*args, site_summary=tsv, site_histogram="32:-4:4", site_table_in=(bins8,))
    assert not os.path.exists(out) and not os.path.exists(tsv)
    # the checks themselves: a run without histograms takes a file with them; a bound left open is compared later
    U.check_site_control(U.load_site_table(bins8), bins8, ["chrA"], [100], None, flag="--site-table-in")
    U.check_site_control(U.load_site_table(bins8), bins8, ["chrA"], [100], (8, None, None), flag="--site-table-in")
    with pytest.raises(ValueError, match="bit for bit"):
        U.check_site_control(U.load_site_table(bins8), bins8, ["chrA"], [100], (8, -4.0, np.nextafter(4.0, 5.0)), flag="--site-table-in")


def test_save_site_table_packed_route_and_merge_by_key():
    """utils on a stand-in handle: packed=True asks the pack alone and keeps the covered sites; merge_site_table hands the file's
    sites over by key, with the totals only when asked"""
    from dynamont_amd.segmentation import utils as U
    import tempfile
    totals = dict(zip(("reads_ok", "rows_added", "samples_added", "rows_without_site", "rows_skipped"), (3, 4, 5, 6, 7)))
    n_rows = np.array([2, 0, 1], dtype=np.uint64)      # the middle record is live by a counter alone: not covered, not saved

    class Fake:
        _site_histogram = (5, -1.0, 1.0)
        merged = None

        def site_table_pack(self, lo, hi):
            assert (lo, hi) == (0, 50)
            return {"site": np.array([4, 9, 40], dtype=np.uint64), "n_rows": n_rows, "limbs": [n_rows * (f + 1) for f in range(7)],
                    "level": np.arange(21, dtype=np.uint32).reshape(3, 7), "dwell": np.ones((3, 16), dtype=np.uint32), "totals": totals}

        def site_summary(self, lo, hi):
            raise AssertionError("the packed route fetches no window")

        def site_summary_merge(self, packed, offset):
            self.merged = (packed, offset)

    path = os.path.join(tempfile.mkdtemp(prefix="sp_"), "t.npz")
    fake = Fake()
    assert U.save_site_table(path, fake, ["chrA"], [50], packed=True) == 2
    t = U.load_site_table(path)
    assert t["site"].tolist() == [4, 40] and t["n_rows"].tolist() == [2, 1] and t["limbs"][6].tolist() == [14, 7] and t["totals"] == totals
    assert t["level"].tolist() == [list(range(7)), list(range(14, 21))] and t["hist_spec"] == (5, -1.0, 1.0)
    assert U.merge_site_table(fake, t, offset=50) == 2
    packed, offset = fake.merged
    assert offset == 50 and packed["site"].tolist() == [4, 40] and packed["totals"] is None and packed["level"].shape == (2, 7)
    assert packed["edges"].tobytes() == (-1.0 + np.arange(6, dtype=np.float64) * (2.0 / 5)).tobytes()
    U.merge_site_table(fake, t, totals=True)
    assert fake.merged[0]["totals"] == totals and fake.merged[1] == 0
    fake._site_histogram = None                         # a handle without histograms takes the table alone
    U.merge_site_table(fake, t)
    assert "level" not in fake.merged[0]
