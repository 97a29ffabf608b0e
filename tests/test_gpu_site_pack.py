"""GPU (-m gpu): the per-site table by content (Aligner.site_table_pack / site_summary_merge, site_pack_kernels.hpp).
  1 - 9    the product's kernels on tables of the test's own (tests/device_math/site_pack.hip, built with the product's flags): every
           integer against the Python-int restatement (tests/site_pack_cases.py), a sparse table's map against what must hold of any
           map (tests/site_map_cases.py: check_map);
  10 - 15  whole reads: a packed table merged into an empty handle is that table, bit for bit, dense or sparse on either side; reads
           split over two handles and merged are all reads on one; the seam of the 2^20-row windows; the files of the packed route;
           a pack while tickets are in flight; what is refused;
  16       the C entry points called directly: a pack over two windows of rows, a merge of more than one chunk of records.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import site_map_cases as smc
import site_pack_cases as spc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native, synth
from dynamont_amd.segmentation import utils as U
from test_gpu_site_summary import NUM_SITES, make_ids, polya_reads

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
BINS = 5                      # bins + 2 + 16 = 23 counters per row: no multiple of the 16 lanes of a row
W = spc.width(BINS)
TOTALS = ("reads_ok", "rows_added", "samples_added", "rows_without_site", "rows_skipped")


# ---- the device harness ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("spack") / "libspack.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_pack.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    for f in (lib.sph_home, lib.sph_probe_max, lib.sph_chunk_rows, lib.sph_scan_tile_rows, lib.sph_lanes):
        f.restype = C.c_uint32
    lib.sph_home_many.restype = None
    assert lib.sph_probe_max() == smc.PROBE_MAX and lib.sph_lanes() == 16
    assert lib.sph_chunk_rows() == spc.CHUNK_ROWS and lib.sph_scan_tile_rows() == spc.SCAN_TILE_ROWS
    return lib


class Table:
    """one table of the harness, dense (capacity = 0) or behind a map: set, pack, merge, window, raw"""

    def __init__(self, lib, num_sites, capacity=0, bins=BINS):
        self.lib, self.num_sites, self.capacity, self.bins = lib, num_sites, capacity, bins
        self.rows, self.W = capacity or num_sites, spc.width(bins)
        self.h = C.c_void_p()
        rc = lib.sph_create(C.c_uint32(num_sites), C.c_uint32(capacity), C.c_uint32(bins), C.byref(self.h))
        assert rc == 0, ("sph_create", rc)

    def home(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(ids.size, dtype=np.uint32)
        self.lib.sph_home_many(p(ids), C.c_uint64(ids.size), C.c_uint32(self.capacity), p(out))
        return out

    def close(self):
        assert self.lib.sph_destroy(self.h) == 0

    def set(self, keys, cells, hist):
        keys = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint32)
        cells = np.ascontiguousarray(cells, dtype=np.uint64)
        hist = None if not self.W else np.ascontiguousarray(hist, dtype=np.uint32)
        assert cells.shape == (self.rows, 7) and (hist is None or hist.shape == (self.rows, self.W))
        rc = self.lib.sph_set(self.h, p(keys), p(cells), p(hist))
        assert rc == 0, ("sph_set", rc)

    def pack(self, row_lo, count, site_lo=0, site_hi=None, cap=None):
        """(total, [(id, words, counters)]) of the first min(total, cap) records"""
        cap = count if cap is None else cap
        site = np.full(max(cap, 1), 0xdeadbeef, dtype=np.uint32)
        cells = np.full((max(cap, 1), 7), 0xdeadbeef, dtype=np.uint64)
        cnt = np.full((max(cap, 1), max(self.W, 1)), 0xdeadbeef, dtype=np.uint32)
        total = C.c_uint64(12345)
        rc = self.lib.sph_pack(self.h, C.c_uint32(row_lo), C.c_uint32(count), C.c_uint32(site_lo),
                               C.c_uint32(self.num_sites if site_hi is None else site_hi), C.c_uint64(cap), p(site), p(cells), p(cnt),
                               C.byref(total))
        assert rc == 0, ("sph_pack", rc)
        n = min(int(total.value), cap)
        return int(total.value), site[:n].copy(), cells[:n].copy(), (cnt[:n, :self.W].copy() if self.W else np.zeros((n, 0), dtype=np.uint32))

    def merge(self, site, cells, counters=None, offset=0, totals=None):
        site = np.ascontiguousarray(site, dtype=np.uint32)
        cells = np.ascontiguousarray(cells, dtype=np.uint64)
        counters = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint32)
        totals = None if totals is None else np.ascontiguousarray(totals, dtype=np.uint64)
        assert cells.shape == (site.size, 7) and (counters is None or counters.shape == (site.size, self.W))
        rc = self.lib.sph_merge(self.h, C.c_uint32(site.size), p(site), C.c_uint64(offset), p(cells), p(counters), p(totals))
        assert rc == 0, ("sph_merge", rc)

    def window(self, lo, count):
        acc = np.full((count, 7), 0xdeadbeef, dtype=np.uint64)
        cnt = np.full((count, self.W), 0xdeadbeef, dtype=np.uint32) if self.W else None
        rc = self.lib.sph_window(self.h, C.c_uint32(lo), C.c_uint32(count), p(acc), p(cnt))
        assert rc == 0, ("sph_window", rc)
        return acc, cnt

    def raw(self):
        """keys (None: dense), cells [rows, 7], totals, stats, hist [rows, W] -- and a map checked"""
        keys = np.zeros(self.capacity, dtype=np.uint32) if self.capacity else None
        acc = np.zeros(self.rows * 7 + 8, dtype=np.uint64)
        hist = np.zeros((self.rows, self.W), dtype=np.uint32) if self.W else None
        rc = self.lib.sph_raw(self.h, p(keys), p(acc), p(hist))
        assert rc == 0, ("sph_raw", rc)
        cells = acc[:self.rows * 7].reshape(self.rows, 7)
        totals = [int(v) for v in acc[self.rows * 7:self.rows * 7 + 5]]
        stats = dict(zip(("n_keys", "rows_dropped", "sites_dropped"), (int(v) for v in acc[self.rows * 7 + 5:])))
        where = None
        if self.capacity:
            where = smc.check_map(keys, cells, stats["n_keys"], self.home)
            if hist is not None:
                assert not hist[keys == smc.EMPTY].any()
        return keys, cells, totals, stats, hist, where


def assert_records(got, want, w, what=""):
    total, site, cells, cnt = got
    ws, wc, wh = spc.records_as_arrays(want, w)
    assert total == len(want), (what, total, len(want))
    assert np.array_equal(site, ws), (what, "site", site[:8], ws[:8])
    assert np.array_equal(cells, wc), (what, "cells", np.argwhere(cells != wc)[:4])
    assert np.array_equal(cnt, wh), (what, "counters", np.argwhere(cnt != wh)[:4])


def assert_table(t, want, what=""):
    """the restated {id: (words, counters)} is the table: every id's row, and nothing else anywhere"""
    keys, cells, _, stats, hist, where = t.raw()
    live = {k: v for k, v in want.items()}
    if t.capacity:
        assert set(live) <= set(where), (what, sorted(set(live) - set(where))[:5])
        rows = {k: where[k] for k in where}
    else:
        rows = {k: k for k in range(t.rows)}
    for k, row in rows.items():
        w, c = live.get(k, ([0] * 7, [0] * t.W))
        assert [int(v) for v in cells[row]] == w, (what, k, [hex(int(v)) for v in cells[row]], [hex(v) for v in w])
        if t.W:
            assert hist[row].tolist() == (c if c else [0] * t.W), (what, k)
    return keys, cells, stats, hist, where


ROWS = (0, 1, 16, 17, spc.SCAN_TILE_ROWS + 1)   # one block's sites and one more; one row more than a step of the scan covers


@pytest.mark.parametrize("rows", ROWS)
def test_1_pack_dense_every_shape_and_pattern(lib, rows):
    """a dense table of `rows` rows and 23 counters a row, its live rows none, all, alternating, only the last: the records are the
    restatement's, in ascending row order, the same bytes from a second launch; a window that starts inside the table"""
    rng = np.random.default_rng(rows)
    t = Table(lib, max(rows, 1))
    for pattern in spc.LIVE_PATTERNS:
        live = spc.live_pattern(pattern, max(rows, 1))
        if rows == 0:
            live[:] = pattern == "all"                                  # (a table has a row; the window of no rows sees none of it)
        cells, hist = spc.random_rows(rng, max(rows, 1), W, live)
        t.set(None, cells, hist)
        want = spc.pack_reference(None, cells, hist, 0, rows, 0, t.num_sites)
        assert len(want) == int(live[:rows].sum())
        first = t.pack(0, rows)
        assert_records(first, want, W, pattern)
        assert (np.diff(first[1].astype(np.int64)) > 0).all()
        again = t.pack(0, rows)
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(first[1:], again[1:])) and again[0] == first[0]
        if rows >= 17:
            assert_records(t.pack(3, rows - 5), spc.pack_reference(None, cells, hist, 3, rows - 5, 0, t.num_sites), W, pattern + " from row 3")
            assert_records(t.pack(0, rows, 5, rows - 1), spc.pack_reference(None, cells, hist, 0, rows, 5, rows - 1), W, pattern + " ids 5 ..")
            total, site, _, _ = t.pack(0, rows, cap=1)                   # fewer records asked for than there are: the count is whole
            assert total == len(want) and site.size == min(1, total)
    t.close()


def test_2_rows_live_by_one_word(lib):
    """a row whose only non-zero word is m2_hi, one whose only non-zero word is the last dwell counter, one live by word 0; with and
    without the counters"""
    cells = np.zeros((17, 7), dtype=np.uint64)
    hist = np.zeros((17, W), dtype=np.uint32)
    cells[2, 6] = 1 << 63
    hist[9, W - 1] = 1
    cells[16, 0] = 1
    t = Table(lib, 17)
    t.set(None, cells, hist)
    want = spc.pack_reference(None, cells, hist, 0, 17, 0, 17)
    assert [r[0] for r in want] == [2, 9, 16]
    assert_records(t.pack(0, 17), want, W)
    t.close()
    t = Table(lib, 17, bins=0)                                          # the table alone: the counters make no row live
    t.set(None, cells, None)
    got = t.pack(0, 17)
    assert_records(got, spc.pack_reference(None, cells, None, 0, 17, 0, 17), 0)
    assert got[1].tolist() == [2, 16]
    t.close()


def test_3_pack_sparse_keys_filter_and_order(lib):
    """a map of 200 buckets, ids up to 4 294 967 293: empty buckets, buckets with a key and all-zero words (not emitted), the id
    filter with a key equal to site_hi and one equal to site_lo; the records stand in bucket order"""
    rng = np.random.default_rng(3)
    cap = 200
    keys = np.full(cap, smc.EMPTY, dtype=np.uint32)
    occupied = np.sort(rng.choice(cap, 120, replace=False))
    ids = np.unique(rng.integers(4000000000, smc.ID_SPACE, 400, dtype=np.uint64))[:117]
    assert ids.size == 117
    keys[occupied] = np.concatenate([ids, [0, 1000, 2000]]).astype(np.uint32)[rng.permutation(120)]
    live = np.zeros(cap, dtype=bool)
    live[occupied] = True
    key_only = occupied[::7]
    live[key_only] = False                                              # k_site_model_scatter leaves such keys
    cells, hist = spc.random_rows(rng, cap, W, live)
    t = Table(lib, smc.ID_SPACE, cap)
    t.set(keys, cells, hist)
    want = spc.pack_reference(keys, cells, hist, 0, cap, 0, smc.ID_SPACE)
    assert len(want) == 120 - key_only.size and max(r[0] for r in want) >= 4000000000
    got = t.pack(0, cap)
    assert_records(got, want, W, "all ids")
    assert not set(got[1].tolist()) & set(keys[key_only].tolist())
    assert (np.diff(got[1].astype(np.int64)) < 0).any()                 # bucket order is not id order
    again = t.pack(0, cap)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[1:], again[1:]))
    some = sorted(r[0] for r in want if r[0] >= 4000000000)
    lo, hi = some[3], some[40]                                          # both are keys of live rows: lo is inside, hi is not
    part = t.pack(0, cap, lo, hi)
    assert_records(part, spc.pack_reference(keys, cells, hist, 0, cap, lo, hi), W, "filtered")
    assert lo in part[1] and hi not in part[1] and part[0] == 37
    assert_records(t.pack(50, 100, 0, 4000000000), spc.pack_reference(keys, cells, hist, 50, 100, 0, 4000000000), W, "buckets 50 .. 149")
    assert t.pack(0, cap, 5, 5)[0] == 0
    t.close()


@pytest.mark.parametrize("capacity", [0, 64], ids=["dense", "sparse"])
def test_4_merge_one_id_a_thousand_times(lib, capacity):
    """ONE launch, 1 000 records of one id between records of two others: every sum exact (the 128-bit ones with carries out of
    the low limb), the totals added once"""
    rng = np.random.default_rng(4)
    n = 1000
    site = np.full(n + 2, 777, dtype=np.uint32)
    site[0], site[-1] = 5, 900
    cells = rng.integers(0, 1 << 64, (n + 2, 7), dtype=np.uint64)
    cells[:, 4] = rng.integers(0, 1 << 20, n + 2)                       # (high limbs: small, and a few negative sums)
    cells[::9, 4] = spc.M64
    cnt = rng.integers(0, 1 << 23, (n + 2, W), dtype=np.uint32)
    records = [(int(site[i]), [int(v) for v in cells[i]], cnt[i].tolist()) for i in range(n + 2)]
    want = {}
    assert spc.merge_reference(want, records) == 0
    assert want[777][0][4] != sum(int(v) for v in cells[1:-1, 4]) & spc.M64          # carries reached m1_hi
    t = Table(lib, 1000, capacity)
    t.merge(site, cells, cnt, totals=[1, 2, 3, 4, 5])
    _, _, stats, _, _ = assert_table(t, want)
    assert t.raw()[2] == [1, 2, 3, 4, 5] and stats["sites_dropped"] == 0 and stats["n_keys"] == (3 if capacity else 0)
    t.close()


@pytest.mark.parametrize("capacity", [0, 16], ids=["dense", "sparse"])
def test_5_carry_and_wrap(lib, capacity):
    """m1_lo = 2^64 - 1 merged twice -- as two records of one launch and again as a second launch --: the carry reaches m1_hi; M2 = -1
    stays a sign-extended -k; a counter wraps mod 2^32; an all-zero record takes no row"""
    M = spc.M64
    rec = (3, [1, 1, 1, M, 0, M, M], [0xFFFFFFFF] + [0] * (W - 2) + [2])
    zero = (8, [0] * 7, [0] * W)
    site, cells, cnt = spc.records_as_arrays([rec, zero, rec], W)
    t = Table(lib, 10, capacity)
    t.merge(site, cells, cnt)
    want = {}
    spc.merge_reference(want, [rec, zero, rec])
    assert want[3][0][3:] == [M - 1, 1, M - 1, M] and want[3][1][0] == 0xFFFFFFFE and 8 not in want
    assert_table(t, want, "one launch")
    t.merge(site, cells, cnt)
    spc.merge_reference(want, [rec, zero, rec])
    assert want[3][0][3:] == [M - 3, 3, M - 3, M] and want[3][1][0] == 0xFFFFFFFC and want[3][1][W - 1] == 8
    _, _, stats, _, _ = assert_table(t, want, "two launches")
    assert stats["n_keys"] == (1 if capacity else 0)
    t.close()


@pytest.mark.parametrize("capacity", [0, 512], ids=["dense", "sparse"])
def test_6_offset_into_the_second_half(lib, capacity):
    N = 100
    rng = np.random.default_rng(6)
    site = rng.permutation(N)[:60].astype(np.uint32)
    site[0], site[1] = 0, N - 1
    cells, cnt = spc.random_rows(rng, 60, W, np.ones(60, dtype=bool))
    t = Table(lib, 2 * N, capacity)
    t.merge(site, cells, cnt, offset=N)
    want = {}
    spc.merge_reference(want, [(int(site[i]), [int(v) for v in cells[i]], cnt[i].tolist()) for i in range(60)], offset=N)
    assert min(want) >= N and max(want) == 2 * N - 1 and N in want
    assert_table(t, want)
    acc, _ = t.window(0, N)
    assert not acc.any()
    site1 = np.array([N], dtype=np.uint32)                              # an id at num_sites - offset: outside, refused by the harness as by the call
    assert lib.sph_merge(t.h, C.c_uint32(1), p(site1), C.c_uint64(N), p(cells[:1].copy()), None, None) == -1
    t.close()


def test_7_probe_wraps_past_the_last_bucket(lib):
    """100 new ids whose home bucket is 1 000 of 1 024, three records each in one launch: the probe sequences wrap past bucket 1 023"""
    t = Table(lib, 1 << 22, 1024)
    ids = smc.same_home_ids(lambda i, c: t.home(i), 1024, 1000, 100)
    rng = np.random.default_rng(7)
    site = np.repeat(np.array(ids, dtype=np.uint32), 3)[rng.permutation(300)]
    cells, cnt = spc.random_rows(rng, 300, W, np.ones(300, dtype=bool))
    t.merge(site, cells, cnt)
    want = {}
    spc.merge_reference(want, [(int(site[i]), [int(v) for v in cells[i]], cnt[i].tolist()) for i in range(300)])
    _, _, stats, _, where = assert_table(t, want)
    assert stats == {"n_keys": 100, "rows_dropped": 0, "sites_dropped": 0}
    assert sorted(where.values()) == sorted((1000 + i) % 1024 for i in range(100))   # buckets 1000 .. 1023, then 0 .. 75: wrapped
    # ... and the pack of that map gives every id's sums back, once
    total, psite, pcells, pcnt = t.pack(0, 1024)
    assert total == 100 and sorted(psite.tolist()) == sorted(ids)
    for i, k in enumerate(psite.tolist()):
        assert [int(v) for v in pcells[i]] == want[k][0] and pcnt[i].tolist() == want[k][1]
    t.close()


def test_8_capacity_four_six_ids(lib):
    """six distinct ids, one record each, into a map of four rows: at most four keys; sites_dropped equals the ids without a bucket;
    no word of a dropped id is anywhere in the table; the kept ids are complete. Then three more records of every id in one
    launch: the kept ids take them, the counter moves by the RECORDS of the ids without a bucket (it counts records)"""
    rng = np.random.default_rng(8)
    ids = [11, 4000000000, 3, 77, 500000, 4294967293]
    site = np.array(ids, dtype=np.uint32)[rng.permutation(6)]
    cells, cnt = spc.random_rows(rng, 6, W, np.ones(6, dtype=bool))
    t = Table(lib, smc.ID_SPACE, 4)
    t.merge(site, cells, cnt, totals=[9, 8, 7, 6, 5])
    keys = t.raw()[0]
    present = set(int(k) for k in keys[keys != smc.EMPTY])
    assert present <= set(ids) and len(present) == 4
    want = {}
    records = [(int(site[i]), [int(v) for v in cells[i]], cnt[i].tolist()) for i in range(6)]
    dropped = spc.merge_reference(want, records, present=present)
    assert dropped == 2 == len(set(ids) - present) and set(want) == present
    _, got_cells, stats, hist, where = assert_table(t, want)            # every row: a kept id's complete sums, or zeros
    assert stats == {"n_keys": 4, "rows_dropped": 0, "sites_dropped": 2} and t.raw()[2] == [9, 8, 7, 6, 5]
    site3 = np.repeat(np.array(ids, dtype=np.uint32), 3)[rng.permutation(18)]
    cells3, cnt3 = spc.random_rows(rng, 18, W, np.ones(18, dtype=bool))
    t.merge(site3, cells3, cnt3)
    assert spc.merge_reference(want, [(int(site3[i]), [int(v) for v in cells3[i]], cnt3[i].tolist()) for i in range(18)], present=present) == 6
    _, got_cells, stats, _, _ = assert_table(t, want, "three more records of every id")
    assert stats == {"n_keys": 4, "rows_dropped": 0, "sites_dropped": 2 + 6} and t.raw()[2] == [9, 8, 7, 6, 5]
    assert int(got_cells[:, 0].sum()) == sum(w[0] for w, _ in want.values()) & spc.M64
    t.close()


def test_9_dense_and_sparse_give_the_same_windows(lib):
    """the same 3 000 records (ids drawn with repeats) into a dense table and into a map: the same windows (k_site_gather), the
    restatement's; the pack of either merged into a third table is that table again"""
    rng = np.random.default_rng(9)
    N = 5000
    site = rng.integers(0, N, 3000).astype(np.uint32)
    cells, cnt = spc.random_rows(rng, 3000, W, rng.random(3000) < 0.9)   # (a tenth of the records all-zero)
    want = {}
    spc.merge_reference(want, [(int(site[i]), [int(v) for v in cells[i]], cnt[i].tolist()) for i in range(3000)])
    dense, sparse = Table(lib, N), Table(lib, N, 4096)
    for t in (dense, sparse):
        t.merge(site, cells, cnt)
    d_acc, d_cnt = dense.window(0, N)
    s_acc, s_cnt = sparse.window(0, N)
    assert d_acc.tobytes() == s_acc.tobytes() and d_cnt.tobytes() == s_cnt.tobytes()
    for k in range(N):
        w, c = want.get(k, ([0] * 7, [0] * W))
        assert [int(v) for v in d_acc[k]] == w and d_cnt[k].tolist() == c, k
    assert sparse.raw()[3]["n_keys"] == len(want)
    for src in (dense, sparse):
        total, psite, pcells, pcnt = src.pack(0, src.rows)
        assert total == len(want)
        third = Table(lib, N, 4096)                                       # (about 2 100 distinct ids: room for all of them)
        third.merge(psite, pcells, pcnt)
        assert third.raw()[3] == {"n_keys": len(want), "rows_dropped": 0, "sites_dropped": 0}
        t_acc, t_cnt = third.window(0, N)
        assert t_acc.tobytes() == d_acc.tobytes() and t_cnt.tobytes() == d_cnt.tobytes()
        third.close()
    dense.close()
    sparse.close()


# ---- whole reads -------------------------------------------------------------------------------------------------------------------
SPEC = (32, -4.0, 4.0)
PROBS = (0.1, 0.5, 0.9)


def bits(v):
    v = np.asarray(v)
    if v.dtype == object:
        return [int(x) for x in v.ravel()]
    return np.ascontiguousarray(v).tobytes()


def table_of(al, lo=0, hi=None):
    """everything the window calls return for [lo, hi), as comparable bits"""
    s, h, q = al.site_summary(lo, hi), al.site_histogram(lo, hi), al.site_quantiles(PROBS, lo, hi)
    out = {"limbs": [bits(c) for c in s["limbs"]], "M1": bits(s["M1"]), "M2": bits(s["M2"]), "totals": s["totals"],
           "level": bits(h["level"]), "dwell": bits(h["dwell"]), "edges": bits(h["edges"])}
    out.update({"q_" + k: bits(q[k]) for k in ("n", "rank", "bin", "below", "in_bin")})
    return out


def handle(models, capacity=None, num_sites=NUM_SITES, spec=SPEC):
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(num_sites, capacity=capacity)
    if spec:
        al.set_site_histogram(*spec)
    return al


@pytest.fixture(scope="module")
def reads48(models):
    reads = polya_reads(models)
    return [r.signal for r in reads], [r.sequence for r in reads], make_ids(reads, 21)


@pytest.fixture(scope="module")
def filled(models, reads48):
    """the 48 poly(A) reads on a dense handle, one launch per batch: (its table, its packed table)"""
    sig, seq, ids = reads48
    al = handle(models)
    al.align_batch(sig, seq, True, site_ids=np.concatenate(ids))
    out = table_of(al), al.site_table_pack()
    assert out[1]["site"].size > 500 and out[0]["totals"]["reads_ok"] == 48
    al.close()
    return out


def assert_packed_equal(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "limbs":
            assert all(bits(x) == bits(y) for x, y in zip(a[k], b[k]))
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("cap_a,cap_b", [(None, None), (None, 8192), (8192, None), (8192, 4096)], ids=["dense_dense", "dense_sparse", "sparse_dense", "sparse_sparse"])
def test_10_copy(models, reads48, filled, cap_a, cap_b):
    """B.site_summary_merge(A.site_table_pack()) makes an empty B equal to A in site_summary, site_histogram, site_quantiles and the
    totals, bit for bit; a dense and a sparse A return equal packed tables"""
    sig, seq, ids = reads48
    want, want_packed = filled
    A, B = handle(models, cap_a), handle(models, cap_b)
    A.align_batch(sig, seq, True, site_ids=np.concatenate(ids))
    packed = A.site_table_pack()
    assert_packed_equal(packed, want_packed)
    assert packed["site"].dtype == np.uint64 and (np.diff(packed["site"].astype(np.int64)) > 0).all()
    assert np.array_equal(packed["site"], np.flatnonzero(A.site_summary()["n_rows"]))
    B.site_summary_merge(packed)
    assert table_of(B) == want == table_of(A)
    if cap_b:
        assert B.site_map() == {"capacity": cap_b, "n_keys": packed["site"].size, "rows_dropped": 0, "sites_dropped": 0}
    # a part of the id range, relative to its start, merged back where it came from: twice the table there, once elsewhere
    part = A.site_table_pack(700, 1500)
    keep = (want_packed["site"] >= 700) & (want_packed["site"] < 1500)
    assert np.array_equal(part["site"] + np.uint64(700), want_packed["site"][keep]) and part["totals"] == want["totals"]
    B.site_summary_merge(dict(part, totals=None), offset=700)
    twice = B.site_summary()
    once = A.site_summary()
    inside = (np.arange(NUM_SITES) >= 700) & (np.arange(NUM_SITES) < 1500)
    assert np.array_equal(twice["n_rows"], once["n_rows"] * np.where(inside, 2, 1).astype(np.uint64)) and twice["totals"] == once["totals"]
    assert [int(v) for v in twice["M2"]] == [int(v) * (2 if i else 1) for v, i in zip(once["M2"], inside)]
    A.close()
    B.close()


@pytest.mark.parametrize("capacity", [None, 8192], ids=["dense", "sparse"])
def test_11_split_over_two_handles_on_tickets(models, reads48, filled, capacity):
    """the rank case without processes: the even reads as a ticket on one handle, the odd reads on another, both packed and merged
    into a third: all reads on one handle"""
    sig, seq, ids = reads48
    want, _ = filled
    target = handle(models, capacity)
    for r in (0, 1):
        part = handle(models, capacity)
        idx = list(range(r, 48, 2))
        packed = synth.pack_reads([synth.SynthRead(sig[i], seq[i]) for i in idx])
        with part.align_async(*packed, True, site_ids=np.concatenate([ids[i] for i in idx])) as t:
            assert (t.wait().status == 0).all()
        target.site_summary_merge(part.site_table_pack())
        part.close()
    assert table_of(target) == want
    target.close()


def test_12_window_seam(models):
    """num_sites = 2^20 + 40 with sites at 2^20 - 1, 2^20 and 2^20 + 39: the last row of the first window of rows, the first and
    the last of the second"""
    N = (1 << 20) + 40
    spec = (BINS, -1.0, 1.0)
    at = [(1 << 20) - 1, 1 << 20, (1 << 20) + 39]
    A = handle(models, None, N, spec)
    edges = A.site_histogram(0, 0)["edges"]
    for j, s in enumerate(at):
        level = np.zeros((1, BINS + 2), dtype=np.uint32)
        level[0, j] = 10 + j
        dwell = np.zeros((1, 16), dtype=np.uint32)
        dwell[0, 15] = 20 + j
        A.site_summary_add(s, {"n_rows": [1 + j], "n_samples": [5], "dwell_sq": [25], "M1": [-(1 << 70) - j], "M2": [(1 << 90) + j]},
                           {"level": level, "dwell": dwell, "edges": edges})
    packed = A.site_table_pack()
    assert packed["site"].tolist() == at and packed["n_rows"].tolist() == [1, 2, 3]
    assert [int(v) for v in packed["M1"]] == [-(1 << 70) - j for j in range(3)] and packed["dwell"][:, 15].tolist() == [20, 21, 22]
    assert A.site_table_pack(1 << 20, N)["site"].tolist() == [0, 39]
    assert A.site_table_pack((1 << 20) - 1, 1 << 20)["site"].tolist() == [0]
    lo = (1 << 20) - 2
    for cap in (None, 64):
        B = handle(models, cap, N, spec)
        B.site_summary_merge(packed)
        assert table_of(B, lo, N) == table_of(A, lo, N)
        assert not B.site_summary(0, lo)["n_rows"].any()
        assert_packed_equal(B.site_table_pack(), packed)
        B.close()
    A.close()


@pytest.mark.parametrize("capacity", [None, 8192], ids=["dense", "sparse"])
def test_13_files(models, reads48, tmp_path, capacity):
    """save_site_table(packed=True) writes arrays equal to the default route's; merge_site_table brings the file back by key"""
    sig, seq, ids = reads48
    al = handle(models, capacity)
    al.align_batch(sig, seq, True, site_ids=np.concatenate(ids))
    a, b = str(tmp_path / "windows.npz"), str(tmp_path / "packed.npz")
    n = U.save_site_table(a, al, ["chrA", "chrB"], [1000, 2000])
    assert U.save_site_table(b, al, ["chrA", "chrB"], [1000, 2000], packed=True) == n > 500
    with np.load(a) as za, np.load(b) as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), k
    back = handle(models, 4096)
    assert U.merge_site_table(back, U.load_site_table(b), totals=True) == n
    assert table_of(back) == table_of(al)
    al.close()
    back.close()


@pytest.mark.parametrize("session", [None, False], ids=["default_mode", "one_launch_per_batch"])
def test_14_pack_while_tickets_are_in_flight(models, reads48, filled, session):
    """four tickets are submitted and the pack is called at once, nothing waited for: it returns the table behind ALL of them --
    what the pack returns once every ticket has been waited for, which is the table of the 48 reads on one handle"""
    sig, seq, ids = reads48
    want, want_packed = filled
    al = handle(models)
    if session is not None:
        al.set_session_mode(session)
    tickets = []
    for j in range(4):
        idx = list(range(j, 48, 4))
        packed = synth.pack_reads([synth.SynthRead(sig[i], seq[i]) for i in idx])
        tickets.append(al.align_async(*packed, True, site_ids=np.concatenate([ids[i] for i in idx])))
    during = al.site_table_pack()                                        # the tickets are in flight: none has been waited for
    for t in tickets:
        assert (t.wait().status == 0).all()
        t.close()
    after = al.site_table_pack()
    assert_packed_equal(during, after)
    assert_packed_equal(after, want_packed)
    assert table_of(al) == want
    al.close()


def test_15_refusals(models, filled):
    _, packed = filled
    al = handle(models)
    n = NUM_SITES
    with pytest.raises(ValueError, match=r"site_summary_merge: record 0: id %d \+ offset 0 is not below the table's %d sites" % (n, n)):
        al.site_summary_merge(dict(packed, site=np.array([n], dtype=np.uint64), limbs=[c[:1] for c in packed["limbs"]], level=packed["level"][:1],
                                   dwell=packed["dwell"][:1]))
    last = int(packed["site"][-1])
    with pytest.raises(ValueError, match=r"record %d: id %d \+ offset %d is not below" % (packed["site"].size - 1, last, n - last)):
        al.site_summary_merge(packed, offset=n - last)                  # an id at num_sites - offset; nothing was added
    assert not al.site_summary()["n_rows"].any() and not any(al.site_summary(0, 0)["totals"].values())
    al.site_summary_merge(packed, offset=n - last - 1)                  # the last id on the last site
    assert int(al.site_summary()["n_rows"][n - 1]) == int(packed["n_rows"][-1])
    with pytest.raises(ValueError, match="level and dwell counters are given together or not at all"):
        al.site_summary_merge({k: v for k, v in packed.items() if k != "dwell"})
    with pytest.raises(ValueError, match="the histogram's edges are not the handle's"):
        al.site_summary_merge(dict(packed, edges=packed["edges"] + 1.0))
    with pytest.raises(ValueError, match="not a range of the table's %d sites" % n):
        al.site_table_pack(0, n + 1)
    empty = al.site_table_pack(5, 5)
    assert empty["site"].size == 0 and empty["level"].shape == (0, SPEC[0] + 2) and len(empty["limbs"]) == 7
    plain = handle(models, spec=None)
    plain._site_histogram = SPEC                                        # (past the wrapper's own check: the C interface refuses)
    with pytest.raises(ValueError, match=r"site_summary_merge: dyn_aligner_set_site_histogram\(a, bins > 0, lo, hi\) was never called"):
        plain.site_summary_merge(packed)
    plain._site_histogram = None
    plain.site_summary_merge({k: v for k, v in packed.items() if k not in ("level", "dwell", "edges", "bins")})   # the table alone
    assert np.array_equal(plain.site_table_pack()["site"], packed["site"]) and "level" not in plain.site_table_pack()
    # a full sparse table: the count in the message, the others added
    small = handle(models, 8)
    with pytest.raises(MemoryError, match=r"site_summary_merge: %d sites found no bucket in the map of 8 rows and were dropped; the other sites were added"
                       % (packed["site"].size - 8)):
        small.site_summary_merge(packed)
    got = small.site_table_pack()
    assert got["site"].size == 8 and small.site_map()["sites_dropped"] == packed["site"].size - 8
    where = np.searchsorted(packed["site"], got["site"])
    assert np.array_equal(packed["site"][where], got["site"]) and np.array_equal(got["n_rows"], packed["n_rows"][where])
    assert np.array_equal(got["level"], packed["level"][where])
    for a in (al, plain, small):
        a.close()
    for call in (lambda: MultiAligner.site_table_pack(None), lambda: MultiAligner.site_summary_merge(None, packed)):
        with pytest.raises(NotImplementedError, match="MultiAligner has no per-site summary"):
            call()


# ---- the C entry points themselves: more than one window of rows, more than one chunk of records ------------------------------
def test_16_c_pack_over_two_windows_and_a_merge_of_more_than_one_chunk(models):
    """dyn_aligner_site_pack over the rows [0, 2^20 + 40) in ONE call (Aligner.site_table_pack asks window by window and never gets
    there): live rows in both windows of rows; arrays too small: the count, nothing copied; arrays that fit: the records in row
    order across the seam. dyn_aligner_site_summary_merge of 2^20 + 7 records in one call (two chunks of staging) with totals:
    every sum exact, the totals added once; no record with totals: the totals alone"""
    N = (1 << 20) + 40
    spec = (BINS, -1.0, 1.0)
    L, P32, P64 = _native.lib(), _native.c_u32_p, _native.c_u64_p
    ptr = lambda a, t: a.ctypes.data_as(t)  # noqa: E731
    al = handle(models, None, N, spec)
    n = (1 << 20) + 7
    rng = np.random.default_rng(16)
    site = rng.integers(0, 5000, n).astype(np.uint32)                    # every id about 200 times, in both chunks
    site[:4] = [0, (1 << 20) - 1, 1 << 20, N - 1]                        # ... and the rows on either side of the seam, the last row
    site[-1] = N - 2                                                     # (a record of the second chunk alone)
    cells = np.zeros((n, 7), dtype=np.uint64)
    cells[:, 0] = 1
    cells[:, 1] = np.arange(n, dtype=np.uint64)
    cells[:, 3] = np.uint64(spc.M64)                                     # M1 += 2^64 - 1 per record: a carry per record but the first
    level = np.zeros((n, BINS + 2), dtype=np.uint32)
    level[np.arange(n), np.arange(n) % (BINS + 2)] = 3
    dwell = np.zeros((n, 16), dtype=np.uint32)
    dwell[:, 15] = 1
    totals = np.array([1, 2, 3, 4, 5], dtype=np.uint64)
    rc = L.dyn_aligner_site_summary_merge(al._h, n, ptr(site, P32), 0, ptr(cells, P64), ptr(totals, P64), ptr(level, P32), ptr(dwell, P32))
    assert rc == _native.DYN_OK, al.last_error()
    rows = np.bincount(site, minlength=N).astype(np.uint64)
    samples = np.zeros(N, dtype=np.uint64)
    np.add.at(samples, site, cells[:, 1])
    live = np.flatnonzero(rows)
    assert live[-2:].tolist() == [N - 2, N - 1] and (live < (1 << 20)).sum() > 4000 and (live >= (1 << 20)).sum() == 3
    # the arrays too small: the count comes back, nothing is copied
    count = np.zeros(1, dtype=np.uint64)
    small_site = np.full(10, 0xdeadbeef, dtype=np.uint32)
    small_cells = np.full((10, 7), 0xdeadbeef, dtype=np.uint64)
    small_level = np.full((10, BINS + 2), 0xdeadbeef, dtype=np.uint32)
    small_dwell = np.full((10, 16), 0xdeadbeef, dtype=np.uint32)
    rc = L.dyn_aligner_site_pack(al._h, 0, N, 0, N, 10, ptr(small_site, P32), ptr(small_cells, P64), ptr(small_level, P32), ptr(small_dwell, P32), ptr(count, P64))
    assert rc == _native.DYN_ERR_INVALID_ARGUMENT and int(count[0]) == live.size
    assert "dyn_aligner_site_pack: %d rows are live, the caller's arrays hold 10" % live.size in al.last_error()
    assert (small_site == 0xdeadbeef).all() and (small_cells == 0xdeadbeef).all() and (small_level == 0xdeadbeef).all() and (small_dwell == 0xdeadbeef).all()
    # the arrays that fit: one call over both windows of rows
    k = live.size
    p_site, p_cells = np.zeros(k, dtype=np.uint32), np.zeros((k, 7), dtype=np.uint64)
    p_level, p_dwell = np.zeros((k, BINS + 2), dtype=np.uint32), np.zeros((k, 16), dtype=np.uint32)
    count[0] = 0
    rc = L.dyn_aligner_site_pack(al._h, 0, N, 0, N, k, ptr(p_site, P32), ptr(p_cells, P64), ptr(p_level, P32), ptr(p_dwell, P32), ptr(count, P64))
    assert rc == _native.DYN_OK and int(count[0]) == k, al.last_error()
    assert np.array_equal(p_site, live)                                  # ascending row across the seam
    assert np.array_equal(p_cells[:, 0], rows[live]) and np.array_equal(p_cells[:, 1], samples[live])
    m1 = [(int(c) * spc.M64) & spc.M128 for c in rows[live]]
    assert [int(v) for v in p_cells[:, 3]] == [v & spc.M64 for v in m1] and [int(v) for v in p_cells[:, 4]] == [v >> 64 for v in m1]
    want_level = np.zeros((N, BINS + 2), dtype=np.uint64)
    np.add.at(want_level, (site, np.arange(n) % (BINS + 2)), 3)
    assert np.array_equal(p_level, want_level[live]) and np.array_equal(p_dwell[:, 15], rows[live]) and not p_dwell[:, :15].any()
    # the Python layer, window by window, returns the same records
    py = al.site_table_pack()
    assert np.array_equal(py["site"], live) and np.array_equal(np.stack(py["limbs"], axis=1), p_cells) and np.array_equal(py["level"], p_level)
    assert list(py["totals"].values()) == [1, 2, 3, 4, 5]               # once, not once per chunk
    # a part of the rows that starts inside the first window and ends inside the second
    count[0] = 0
    rc = L.dyn_aligner_site_pack(al._h, 4000, N - 1, 0, N, k, ptr(p_site, P32), ptr(p_cells, P64), None, None, ptr(count, P64))
    part = live[(live >= 4000) & (live < N - 1)]
    assert rc == _native.DYN_OK and int(count[0]) == part.size and np.array_equal(p_site[:part.size], part)
    assert np.array_equal(p_cells[:part.size, 1], samples[part])
    # no record, totals: the totals alone; no record, no totals: nothing
    assert L.dyn_aligner_site_summary_merge(al._h, 0, None, 0, None, ptr(totals, P64), None, None) == _native.DYN_OK
    assert L.dyn_aligner_site_summary_merge(al._h, 0, None, 0, None, None, None, None) == _native.DYN_OK
    assert list(al.site_summary(0, 0)["totals"].values()) == [2, 4, 6, 8, 10]
    al.site_summary_merge({"site": np.zeros(0, dtype=np.uint64), "limbs": [np.zeros(0, dtype=np.uint64)] * 7, "totals": [1, 1, 1, 1, 1]})
    assert list(al.site_summary(0, 0)["totals"].values()) == [3, 5, 7, 9, 11]
    assert np.array_equal(al.site_table_pack()["site"], live)
    al.close()
