"""GPU (-m gpu): the sparse mode of the per-site table (Aligner.set_site_summary(num_sites, capacity=), site_map.hpp).
  1 - 8   the product's kernels on arrays of the test's own (tests/device_math/site_map.hip, built with the product's flags):
          every integer against the Python-int restatement (tests/site_map_cases.py), the map against what must hold of any map;
  9 - 11  whole reads: a dense and a sparse handle on the same reads return the same bits from every window call; an id space no
          dense table could be allocated for; the switch between the modes while a ticket is in flight.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import site_histogram_cases as shc
import site_map_cases as smc
import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from test_gpu_site_summary import NUM_SITES, make_ids, polya_reads, submit

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


# ---- the device harness ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = tmp_path_factory.mktemp("smap") / "libsmap.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_map.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.smh_home.restype = C.c_uint32
    lib.smh_probe_max.restype = C.c_uint32
    lib.smh_home_many.restype = None
    assert lib.smh_probe_max() == smc.PROBE_MAX
    return lib


def home_of(lib):
    def home(ids, capacity):
        ids = np.ascontiguousarray(ids, dtype=np.uint32)
        out = np.zeros(ids.size, dtype=np.uint32)
        lib.smh_home_many(p(ids), C.c_uint64(ids.size), C.c_uint32(capacity), p(out))
        return out
    return home


class Map:
    """one map of the harness: fill, gather, scatter, windows, raw"""

    def __init__(self, lib, capacity, num_sites=smc.ID_SPACE, spec=None):
        self.lib, self.capacity, self.num_sites, self.spec = lib, capacity, num_sites, spec
        self.bins = spec[0] if spec else 0
        self.H = self.bins + 2 + 16 if spec else 0
        self.h = C.c_void_p()
        lo, inv_w = (spec[1], float(shc.inv_width(*spec))) if spec else (0.0, 0.0)
        rc = lib.smh_create(C.c_uint32(num_sites), C.c_uint32(capacity), C.c_uint32(self.bins), C.c_double(lo), C.c_double(inv_w), C.byref(self.h))
        assert rc == 0, ("smh_create", rc)
        self.home = lambda ids: home_of(lib)(ids, capacity)

    def close(self):
        assert self.lib.smh_destroy(self.h) == 0

    def fill(self, b, runs=1, sync=1, lo=0, hi=None):
        rc = self.lib.smh_fill(self.h, C.c_int(len(b.read)), p(b.sig_off), p(b.par_off), p(b.seg_off), p(b.T), p(b.N), p(b.read),
                               C.c_int(len(b.status)), p(b.status), C.c_uint64(len(b.sig)), p(b.sig), C.c_uint64(len(b.segrow)), p(b.segrow),
                               C.c_uint64(len(b.sites)), p(b.sites), C.c_uint32(lo), C.c_uint32(len(b.reads) if hi is None else hi),
                               C.c_int(runs), C.c_int(sync))
        assert rc == 0, ("smh_fill", rc)

    def gather(self, lo, count, table=True, hist=False, other_stream=0):
        acc = np.full((count, 7), 0xdeadbeef, dtype=np.uint64) if table else None
        cnt = np.full((count, self.H), 0xdeadbeef, dtype=np.uint32) if hist else None
        rc = self.lib.smh_gather(self.h, C.c_uint32(lo), C.c_uint32(count), p(acc) if table else None, p(cnt) if hist else None, C.c_int(other_stream))
        assert rc == 0, ("smh_gather", rc)
        return acc, cnt

    def scatter(self, lo, cols, counters=None, totals=None):
        cols = np.ascontiguousarray(cols, dtype=np.uint64)
        counters = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint32)
        totals = None if totals is None else np.ascontiguousarray(totals, dtype=np.uint64)
        rc = self.lib.smh_scatter(self.h, C.c_uint32(lo), C.c_uint32(len(cols)), p(cols), None if counters is None else p(counters),
                                  None if totals is None else p(totals))
        assert rc == 0, ("smh_scatter", rc)

    def windows(self, shift):
        n_win = ((self.num_sites - 1) >> shift) + 1
        bitmap = np.zeros((n_win + 31) // 32, dtype=np.uint32)
        rc = self.lib.smh_windows(self.h, C.c_int(shift), p(bitmap), C.c_uint64(bitmap.size))
        assert rc == 0, ("smh_windows", rc)
        bits = np.unpackbits(bitmap.view(np.uint8), bitorder="little")
        return np.flatnonzero(bits)

    def raw(self):
        """keys, cells [capacity, 7], totals dict, stats dict, hist [capacity, H] or None -- and the map checked"""
        keys = np.zeros(self.capacity, dtype=np.uint32)
        acc = np.zeros(self.capacity * 7 + 8, dtype=np.uint64)
        hist = np.zeros((self.capacity, self.H), dtype=np.uint32) if self.spec else None
        rc = self.lib.smh_raw(self.h, p(keys), p(acc), None if hist is None else p(hist))
        assert rc == 0, ("smh_raw", rc)
        cells = acc[:self.capacity * 7].reshape(self.capacity, 7)
        totals = dict(zip(ssc.TOTALS, (int(v) for v in acc[self.capacity * 7:self.capacity * 7 + 5])))
        stats = dict(zip(("n_keys", "rows_dropped", "sites_dropped"), (int(v) for v in acc[self.capacity * 7 + 5:])))
        where = smc.check_map(keys, cells, stats["n_keys"], self.home)
        if hist is not None:
            assert not hist[keys == smc.EMPTY].any()
        return keys, cells, totals, stats, hist, where


def assert_cells(m, want, what=""):
    """every key of the map holds exactly the restated cell; every restated cell's key is in the map"""
    keys, cells, totals, stats, hist, where = m.raw()
    assert sorted(where) == sorted(want["cells"]), (what, "keys", len(where), len(want["cells"]))
    for k, c in want["cells"].items():
        got = [int(v) for v in cells[where[k]]]
        assert got == smc.cell_limbs(c), (what, k, [hex(v) for v in got], [hex(v) for v in smc.cell_limbs(c)])
    assert totals == want["totals"], (what, totals, want["totals"])
    return keys, cells, totals, stats, hist, where


@pytest.fixture(scope="module")
def scattered():
    b = ssc.build_batch()
    table = smc.scatter_ids()
    reads = smc.remap(b.reads, table)
    return reads, smc.pack(reads), table


def test_1_scattered_ids(lib, scattered):
    """site_summary_cases' batch (both kernels, 128-bit carries, skipped and site-less rows, a failed read) with its 40 ids sent
    into the whole id space, ids at or above 4 000 000 000 among them, at capacity 64"""
    reads, b, table = scattered
    want, dropped = smc.reference(reads)
    dense = ssc.reference(ssc.build_batch())
    with_rows = [s for s in range(ssc.NUM_SITES) if dense["n_rows"][s]]
    assert dropped == 0 and sorted(want["cells"]) == sorted(table[s] for s in with_rows) and max(want["cells"]) >= 4000000000
    assert want["totals"] == dense["totals"]                                     # the mapping moved ids, nothing else
    m = Map(lib, 64)
    m.fill(b)
    keys, cells, totals, stats, _, where = assert_cells(m, want, "run 1")
    assert stats == {"n_keys": len(with_rows), "rows_dropped": 0, "sites_dropped": 0}
    # the gathered window at each id: the id's cell, its neighbours (absent) zero
    for s in range(ssc.NUM_SITES):
        k = table[s]
        lo = min(max(k - 1, 0), smc.ID_SPACE - 3)
        got, _ = m.gather(lo, 3)
        for i in range(3):
            c = want["cells"].get(lo + i)
            assert [int(v) for v in got[i]] == (smc.cell_limbs(c) if c else [0] * 7), (s, k, lo + i)
    m.fill(b)
    twice, _ = smc.reference(reads, runs=2)
    keys2 = assert_cells(m, twice, "run 2")[0]
    assert np.array_equal(keys, keys2)
    m.close()


def contended(lib, n_keys, capacity, bucket, n_reads, per_wave, seed, long_rows=()):
    ids = smc.same_home_ids(home_of(lib), capacity, bucket, n_keys)
    assert set(home_of(lib)(ids, capacity).tolist()) == {bucket}
    reads = smc.contended_reads(ids, n_reads, per_wave, seed, long_rows)
    return ids, reads, smc.pack(reads)


def test_2_one_home_bucket_under_contention(lib):
    """100 new keys with home bucket 1000 of 1 024: the probe sequences wrap past bucket 1 023. Every key has 64 rows in ONE launch,
    8 consecutive lanes of a wave in each of 8 reads (4 blocks per read), and three keys a row for the block-per-read kernel"""
    ids, reads, b = contended(lib, 100, 1024, 1000, 8, 8, 1, long_rows=((0, 300), (50, 257), (99, 700)))
    want, dropped = smc.reference(reads)
    assert dropped == 0 and min(c[0] for c in want["cells"].values()) >= 64 and len(want["cells"]) == 100
    m = Map(lib, 1024)
    m.fill(b)
    keys, _, _, stats, _, where = assert_cells(m, want)
    assert stats == {"n_keys": 100, "rows_dropped": 0, "sites_dropped": 0}
    assert sorted(where.values()) == sorted((1000 + i) % 1024 for i in range(100))   # buckets 1000 .. 1023, then 0 .. 75: wrapped
    m.close()


def overflow(lib, n_keys, capacity, bucket, n_reads, per_wave, seed):
    ids, reads, b = contended(lib, n_keys, capacity, bucket, n_reads, per_wave, seed)
    m = Map(lib, capacity)
    m.fill(b)
    keys = m.raw()[0]
    present = set(int(k) for k in keys[keys != smc.EMPTY])
    assert present <= set(ids)
    want, dropped = smc.reference(reads, present=present)
    _, _, totals, stats, _, _ = assert_cells(m, want)                            # every present key's cell is complete
    all_rows = sum(len(segs) for _, segs in reads)
    assert stats["rows_dropped"] == dropped == all_rows - sum(c[0] for c in want["cells"].values())
    assert totals["rows_added"] + totals["rows_without_site"] + totals["rows_skipped"] == all_rows
    m.close()
    return stats


def test_3_probe_limit(lib):
    """200 keys with one home at capacity 1 024: the probe window of 128 buckets fills and stays full"""
    stats = overflow(lib, 200, 1024, 500, 2, 4, 2)
    assert stats["n_keys"] == 128 and stats["rows_dropped"] == 72 * 8


def test_4_full_map(lib):
    stats = overflow(lib, 20, 8, 3, 2, 4, 3)
    assert stats["n_keys"] == 8 and stats["rows_dropped"] == 12 * 8


@pytest.mark.parametrize("spec", [shc.EXACT, shc.ROUNDED], ids=["32_exact_width", "30_rounded_width"])
def test_5_histograms_through_the_map(lib, spec):
    """site_histogram_cases' batch (rows on and around every bin edge, dwell bins up to 2^15) through scattered ids"""
    b0 = shc.build_batch()
    table = smc.scatter_ids()
    reads = smc.remap(b0.reads, table)
    hist = {}
    want, _ = smc.reference(reads, hist=hist, spec=spec)
    dense = shc.reference(b0, *spec)
    for s in range(ssc.NUM_SITES):                                               # the dict restatement IS the cases' reference
        lv, dw = hist.get(table[s], ([0] * (spec[0] + 2), [0] * 16))
        assert lv == dense["level"][s] and dw == dense["dwell"][s], s
    m = Map(lib, 97, spec=spec)
    m.fill(smc.pack(reads))
    _, cells, _, stats, got, where = assert_cells(m, want)
    B = spec[0] + 2
    for k, (lv, dw) in hist.items():
        row = got[where[k]]
        assert row[:B].tolist() == lv and row[B:].tolist() == dw, k
        assert int(row[:B].sum()) == int(row[B:].sum()) == int(cells[where[k]][0])   # both groups sum to n_rows
    # the gathered counters of a window that holds a key, and of its absent neighbours
    k = table[11]
    lo = min(max(k - 2, 0), smc.ID_SPACE - 5)
    _, cnt = m.gather(lo, 5, table=False, hist=True)
    for i in range(5):
        lv, dw = hist.get(lo + i, ([0] * B, [0] * 16))
        assert cnt[i].tolist() == lv + dw, (lo + i)
    m.close()


def test_6_scatter_add(lib, scattered):
    """k_site_scatter_add into present keys, into new keys and over all-zero sites; the 128-bit carries; a full map"""
    reads, b, table = scattered
    spec = shc.EXACT
    H = spec[0] + 2 + 16
    hist = {}
    want, _ = smc.reference(reads, hist=hist, spec=spec)
    m = Map(lib, 256, spec=spec)
    m.fill(b)
    n0 = m.raw()[3]["n_keys"]
    # a window of 40 ids around a present key (site 11: M1's low limb near wrapping): the present key, 5 new keys, the rest zero
    k = table[11]
    lo = min(max(k - 20, 0), smc.ID_SPACE - 40)
    rng = np.random.default_rng(5)
    cols = np.zeros((40, 7), dtype=np.uint64)
    cnts = np.zeros((40, H), dtype=np.uint32)
    new = [i for i in rng.permutation(40) if lo + int(i) not in want["cells"]][:5]
    M64 = ssc.M64
    cols[k - lo] = np.array([3, 30, 300, M64, 0, M64 - 5, M64], dtype=np.uint64)   # M1 += 2^64 - 1: carries; M2 += -6, sign-extended
    cnts[k - lo, 1] = 7
    for j, i in enumerate(new):
        cols[i] = np.array([1 + j, 10, 100, M64 - j, 1, 5, 0], dtype=np.uint64)
    cols[new[0]] = 0
    cnts[new[0], H - 1] = 9                                                      # a site with counters alone still inserts
    totals_in = [1, 2, 3, 4, 5]
    m.scatter(lo, cols, cnts, totals_in)
    m.scatter(lo, cols, cnts)                                                    # twice: the second time into present keys only
    for i in range(40):
        if cols[i].any() or cnts[i].any():
            c = want["cells"].setdefault(lo + i, [0] * 5)
            add = smc.from_limbs(cols[i])
            for f in range(5):
                c[f] += 2 * add[f]
            lv, dw = hist.setdefault(lo + i, ([0] * (spec[0] + 2), [0] * 16))
            for w in range(spec[0] + 2):
                lv[w] += 2 * int(cnts[i, w])
            for w in range(16):
                dw[w] += 2 * int(cnts[i, spec[0] + 2 + w])
    for f, name in enumerate(ssc.TOTALS):
        want["totals"][name] += totals_in[f]
    _, _, _, stats, got_hist, where = assert_cells(m, want, "after the adds")
    assert stats["n_keys"] == n0 + 5 and stats["sites_dropped"] == 0             # the 34 all-zero sites inserted nothing
    acc, cnt = m.gather(lo, 40, hist=True)
    for i in range(40):
        c = want["cells"].get(lo + i)
        assert [int(v) for v in acc[i]] == (smc.cell_limbs(c) if c else [0] * 7), i
        lv, dw = hist.get(lo + i, ([0] * (spec[0] + 2), [0] * 16))
        assert cnt[i].tolist() == lv + dw, i
    m.close()
    # a full map: 8 rows, 20 sites with a word each -> 8 get in, 12 are counted, the 8 are added
    m = Map(lib, 8, num_sites=1000)
    cols = np.zeros((20, 7), dtype=np.uint64)
    cols[:, 0] = np.arange(1, 21)
    m.scatter(100, cols)
    keys, cells, _, stats, _, where = m.raw()
    assert stats == {"n_keys": 8, "rows_dropped": 0, "sites_dropped": 12}
    for k, row in where.items():
        assert [int(v) for v in cells[row]] == [k - 100 + 1, 0, 0, 0, 0, 0, 0]
    m.close()


def test_6_site_summary_add_on_a_full_map_reports_the_dropped_sites(models):
    """the product's call on a sparse handle of 8 rows: 20 sites with a word each. 8 get in with their exact sums (the 128-bit
    ones included), 12 are counted and the call raises with the count; a second call reports that call's drops alone"""
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(1000, capacity=8)
    al.set_site_histogram(*SPEC)
    n = 20
    summary = {"n_rows": np.arange(1, n + 1, dtype=np.uint64), "n_samples": np.arange(10, 10 + n, dtype=np.uint64),
               "dwell_sq": np.arange(100, 100 + n, dtype=np.uint64), "M1": [(1 << 64) - 1 - i for i in range(n)],
               "M2": [-(i + 1) for i in range(n)], "totals": [1, 2, 3, 4, 5]}
    level = np.zeros((n, SPEC[0] + 2), dtype=np.uint32)
    level[:, 3] = np.arange(1, n + 1)
    dwell = np.zeros((n, 16), dtype=np.uint32)
    dwell[:, 15] = 7
    hist = {"level": level, "dwell": dwell, "edges": al.site_histogram(0, 0)["edges"]}
    with pytest.raises(MemoryError, match=r"site_summary_add: 12 sites found no bucket in the map of 8 rows and were dropped; the other sites were added"):
        al.site_summary_add(100, summary, hist)
    assert al.site_map() == {"capacity": 8, "n_keys": 8, "rows_dropped": 0, "sites_dropped": 12}
    keys = al.site_map_keys()
    assert np.unique(keys).size == 8 and ((keys >= 100) & (keys < 120)).all()

    def check(times):
        got, h = al.site_summary(100, 120), al.site_histogram(100, 120)
        for i in range(n):
            inside = 100 + i in keys
            k = times if inside else 0
            assert int(got["n_rows"][i]) == k * (i + 1) and int(got["n_samples"][i]) == k * (10 + i) and int(got["dwell_sq"][i]) == k * (100 + i), i
            assert int(got["M1"][i]) == k * ((1 << 64) - 1 - i) and int(got["M2"][i]) == -k * (i + 1), i       # the carry; the sign
            assert int(h["level"][i, 3]) == k * (i + 1) and int(h["level"][i].sum()) == k * (i + 1) and int(h["dwell"][i, 15]) == 7 * k, i
        return got["totals"]

    assert list(check(1).values()) == [1, 2, 3, 4, 5]
    # again, with 3 sites more behind them: the 8 present sites take the sums twice, 12 + 3 sites are dropped by THIS call
    more = {k: (np.concatenate([v, v[:3]]) if isinstance(v, np.ndarray) else v + v[:3]) for k, v in summary.items() if k != "totals"}
    with pytest.raises(MemoryError, match="site_summary_add: 15 sites found no bucket"):
        al.site_summary_add(100, more)
    assert al.site_map() == {"capacity": 8, "n_keys": 8, "rows_dropped": 0, "sites_dropped": 27}
    got = al.site_summary(100, 123)
    assert not got["n_rows"][20:].any() and [int(v) for v in got["n_rows"][:20]] == [2 * (i + 1) if 100 + i in keys else 0 for i in range(n)]
    # all-zero sites insert nothing and drop nothing, full map or not
    al.site_summary_add(500, {k: np.zeros(4, dtype=np.uint64) if k != "M1" and k != "M2" else [0] * 4 for k in ("n_rows", "n_samples", "dwell_sq", "M1", "M2")})
    assert al.site_map()["sites_dropped"] == 27
    al.reset_site_summary()
    al.site_summary_add(100, {k: (v[:5] if k != "totals" else v) for k, v in summary.items()})          # room again: no error
    assert al.site_map() == {"capacity": 8, "n_keys": 5, "rows_dropped": 0, "sites_dropped": 0}
    al.close()


def test_7_occupied_windows(lib):
    rng = np.random.default_rng(7)
    ids = np.unique(np.concatenate([rng.integers(0, smc.ID_SPACE, 300), [0, smc.ID_SPACE - 1], rng.integers(5 << 20, 6 << 20, 50)])).astype(np.uint64)
    m = Map(lib, 1024)
    cols = np.zeros((1, 7), dtype=np.uint64)
    cols[0, 0] = 1
    for k in ids.tolist():
        m.scatter(k, cols)
    assert m.raw()[3]["n_keys"] == ids.size
    assert np.array_equal(m.windows(20), np.unique(ids >> np.uint64(20)))
    m.close()
    small = np.unique(rng.integers(0, 5000, 200)).astype(np.uint64)
    m = Map(lib, 512, num_sites=5000)
    for k in small.tolist():
        m.scatter(k, cols)
    assert np.array_equal(m.windows(4), np.unique(small >> np.uint64(4)))
    assert np.array_equal(m.windows(20), [0])
    m.close()


def test_8_no_tear(lib):
    """ONE gather on a second stream while ONE filling launch is in flight (4 reads of 600 rows of 257 .. 300 samples: the
    block-per-read kernel walks them in order for milliseconds). Each 64-bit field a row adds to is a value that field takes in
    SOME prefix of its adds -- with identical rows, a multiple of the row's term between zero and the final sum"""
    keys = [4000000100, 4000000101, 4000000105, 4000000163]
    x = np.full(300, 0.5)                                                        # m = 0.5, m1 = 2^39, m2 = 2^38: no carries
    reads = [(0, [(keys[(j + r) % 4], x) for j in range(600)]) for r in range(4)]
    m = Map(lib, 32)
    m.fill(smc.pack(reads), sync=0)
    got, _ = m.gather(keys[0], 64, other_stream=1)                               # the one gather: a window that holds the four keys
    seen = {k: [int(v) for v in got[k - keys[0]]] for k in keys}
    assert not got[[i for i in range(64) if keys[0] + i not in keys]].any()
    final, _ = smc.reference(reads)
    term = [1, 300, 90000, 1 << 39, 0, 1 << 38, 0]
    for k in keys:
        n = final["cells"][k][0]
        for f in range(7):
            v = seen[k][f]
            assert (v == 0) if term[f] == 0 else (v % term[f] == 0 and 0 <= v // term[f] <= n), (k, f, v)
    assert_cells(m, final)
    print("rows seen by the gather:", {k: seen[k][0] for k in keys}, "of", {k: final["cells"][k][0] for k in keys})
    m.close()


# ---- whole reads: a dense and a sparse handle ------------------------------------------------------------------------------------
SPEC = (32, -4.0, 4.0)
PROBS = (0.1, 0.5, 0.9)


def window_calls(al, lo, hi, other):
    n = hi - lo
    out = {"summary": al.site_summary(lo, hi), "histogram": al.site_histogram(lo, hi), "quantiles": al.site_quantiles(PROBS, lo, hi)}
    if other is not None:
        out["compare"] = al.site_compare(lo, hi, other)
        out["mixture"] = al.site_mixture(lo, hi, other)
        assert n > 0
    return out


def bits(v):
    v = np.asarray(v)
    if v.dtype == object:
        return [int(x) for x in v.ravel()]
    return np.ascontiguousarray(v).tobytes()


def assert_same_bits(a, b, what=""):
    assert a.keys() == b.keys()
    for call in a:
        assert a[call].keys() == b[call].keys(), (what, call)
        for name, v in a[call].items():
            w = b[call][name]
            if isinstance(v, (list, tuple)) and len(v) and isinstance(v[0], np.ndarray):
                assert all(bits(x) == bits(y) for x, y in zip(v, w)), (what, call, name)
            elif isinstance(v, np.ndarray):
                assert v.dtype == w.dtype and v.shape == w.shape and bits(v) == bits(w), (what, call, name)
            else:
                assert v == w, (what, call, name)


@pytest.fixture(scope="module")
def tickets(models):
    """the four tickets of the dense table's test (the 48 polyA reads repeated to 512 reads, ticket j from read 7 j, ids of its
    own), without their restatement, and the dense table of each from a handle of its own: (packed, ids, dense summary)"""
    reads = polya_reads(models)
    out = []
    for j in range(4):
        ids48 = make_ids(reads, 10 + j)
        idx = [(7 * j + i) % 48 for i in range(512)]
        tk = (synth.pack_reads([reads[i] for i in idx]), np.concatenate([ids48[i] for i in idx]), None)
        al = Aligner(models["syn5"], "rna002", device=0)
        al.set_site_summary(NUM_SITES)
        with submit(al, tk) as t:
            t.wait()
        out.append(tk[:2] + (al.site_summary(),))
        al.close()
    return out


def two_handles(models, model, mode, num_sites, capacity, session=None):
    out = []
    for cap in (None, capacity):
        al = Aligner(models[model], mode, device=0)
        if session is not None:
            al.set_session_mode(session)
        al.set_site_summary(num_sites, capacity=cap)
        al.set_site_histogram(*SPEC)
        out.append(al)
    return out


def test_9_same_bits_as_dense_align_batch(models):
    """the 48 reads of the dense table's test; sample ids in [0, N), the same reads again as a control in [N, 2 N)"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6301, 48, "dna_r10_400bps", mean, sd, (40, 400), dwell=13.0)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    N = NUM_SITES
    ids = np.concatenate(make_ids(reads, 1))
    ctl = np.concatenate(make_ids(reads, 2))
    ctl = np.where(ctl < N, ctl + N, ctl).astype(np.uint32)
    dense, sparse = two_handles(models, "syn9", "dna_r10_400bps", 2 * N, 8192)
    for al in (dense, sparse):
        al.align_batch(sig, seq, True, site_ids=ids)
        al.align_batch(sig[:30], seq[:30], True, site_ids=ctl[:sum(len(s) for s in seq[:30])])
    want = window_calls(dense, 0, N, N)
    assert (want["summary"]["n_rows"] > 1).sum() > 500
    assert_same_bits(window_calls(sparse, 0, N, N), want, "[0, N) against [N, 2 N)")
    assert_same_bits(window_calls(sparse, 0, 2 * N, None), window_calls(dense, 0, 2 * N, None), "the whole id space")
    assert_same_bits(window_calls(sparse, 17, 1201, 2 * N - 1184), window_calls(dense, 17, 1201, 2 * N - 1184), "odd windows")
    st = sparse.site_map()
    touched = int((window_calls(dense, 0, 2 * N, None)["summary"]["n_rows"] > 0).sum())
    assert st == {"capacity": 8192, "n_keys": touched, "rows_dropped": 0, "sites_dropped": 0}
    keys = sparse.site_map_keys()
    assert keys.size == 8192 and (keys != 0xFFFFFFFF).sum() == touched and np.unique(keys).size == touched + 1
    assert np.array_equal(sparse.site_map_windows(8), np.unique(keys[keys != 0xFFFFFFFF] >> 8))
    with pytest.raises(ValueError, match="dense"):
        dense.site_map()
    with pytest.raises(ValueError, match="dense"):
        dense.site_map_keys(0, 1)
    with pytest.raises(ValueError, match="dense"):
        dense.site_map_windows()
    # site_summary_add through the map: the sparse table added onto itself is the dense one added onto itself
    s, h = want["summary"], want["histogram"]
    for al in (dense, sparse):
        al.site_summary_add(0, al.site_summary(0, N), al.site_histogram(0, N))
    assert_same_bits(window_calls(sparse, 0, N, N), window_calls(dense, 0, N, N), "after site_summary_add")
    assert np.array_equal(sparse.site_summary(0, N)["n_rows"], 2 * s["n_rows"]) and sparse.site_map()["n_keys"] == touched
    assert np.array_equal(sparse.site_histogram(0, N)["level"], 2 * h["level"])
    # reset empties the keys
    sparse.reset_site_summary()
    assert sparse.site_map() == {"capacity": 8192, "n_keys": 0, "rows_dropped": 0, "sites_dropped": 0}
    assert (sparse.site_map_keys() == 0xFFFFFFFF).all() and not sparse.site_summary()["n_rows"].any()
    assert not sparse.site_histogram()["level"].any() and sparse.site_map_windows().size == 0
    dense.close()
    sparse.close()


def test_9_same_bits_as_dense_four_tickets_that_merge(models, tickets):
    """the merging tickets of the dense table's test on a dense and on a sparse handle of 2 N sites, the third ticket's ids moved
    into the control half [N, 2 N): the same table and the same comparison of the halves, whatever merged"""
    tks = tickets
    N = NUM_SITES
    control = (tks[2][0], np.where(tks[2][1] < N, tks[2][1] + np.uint32(N), tks[2][1]).astype(np.uint32), None)
    tables = []
    for al in two_handles(models, "syn5", "rna002", 2 * N, 4096, session=False):
        al.set_auto_guide(0)
        ahead = submit(al, tks[3], with_ids=False)
        ts = [ahead, submit(al, tks[0]), submit(al, tks[1], with_ids=False), submit(al, control)]
        for t in ts:
            t.wait()
            t.close()
        tables.append(window_calls(al, 0, N, N))
        if al._site_capacity:
            assert al.site_map()["rows_dropped"] == 0
        al.close()
    assert [int(v) for v in tables[0]["summary"]["M1"]] == [int(v) for v in tks[0][2]["M1"]]
    assert tables[0]["compare"]["n_a"].any() and tables[0]["compare"]["n_b"].any()     # both halves hold rows
    assert_same_bits(tables[1], tables[0])


def test_9_same_bits_as_dense_resident_session(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(6302, 600, "rna004", mean, sd, (28, 36))
    packed, flat = synth.pack_reads(reads), np.concatenate(make_ids(reads, 4, span=300))
    N = NUM_SITES
    ctl = np.concatenate(make_ids(reads, 5, span=300))
    ctl = np.where(ctl < N, ctl + np.uint32(N), ctl).astype(np.uint32)       # a second ticket: the control half [N, 2 N)
    tables = []
    for session in (True, False):
        for al in two_handles(models, "syn9", "rna004", 2 * N, 2048, session=session):
            with al.align_async(*packed, True, site_ids=flat) as t:
                t.wait()
                assert t.timing()["launches"] == (0 if session else 1)
            with al.align_async(*packed, True, site_ids=ctl) as t:
                t.wait()
            tables.append(window_calls(al, 0, N, N))
            al.close()
    assert tables[0]["summary"]["totals"]["reads_ok"] == 1200 and tables[0]["compare"]["n_b"].any()
    for i in (1, 2, 3):
        assert_same_bits(tables[i], tables[0], "table %d" % i)


def test_10_beyond_dense(models):
    """num_sites = 4 294 967 294 and ids around 4 x 10^9 at capacity 4 096 (a dense table of that size: 240 GB): every window call"""
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    N = NUM_SITES
    A, B = 4000000000, 4100000000
    # (an id outside [0, N) becomes DYN_SITE_NONE: the small table's second window would hold it, the big one's would not)
    move = lambda ids, off: np.where(ids < N, ids.astype(np.int64) + off, 0xFFFFFFFF).astype(np.uint32)  # noqa: E731
    small = Aligner(models["syn5"], "rna002", device=0)
    small.set_site_summary(2 * N)
    small.set_site_histogram(*SPEC)
    big = Aligner(models["syn5"], "rna002", device=0)
    big.set_site_summary(smc.ID_SPACE, capacity=4096)
    big.set_site_histogram(*SPEC)
    flat = np.concatenate(make_ids(reads, 1))
    ctl = np.concatenate(make_ids(reads, 2))
    small.align_batch(sig, seq, True, site_ids=move(flat, 0))
    small.align_batch(sig, seq, True, site_ids=move(ctl, N))
    big.align_batch(sig, seq, True, site_ids=move(flat, A))
    big.align_batch(sig, seq, True, site_ids=move(ctl, B))
    want = window_calls(small, 0, N, N)
    assert_same_bits(window_calls(big, A, A + N, B), want)
    st = big.site_map()
    assert st["rows_dropped"] == 0 and st["n_keys"] == int((small.site_summary()["n_rows"] > 0).sum())
    wins = big.site_map_windows(20)
    keys = big.site_map_keys()
    assert np.array_equal(wins, np.unique(keys[keys != 0xFFFFFFFF] >> 20)) and A >> 20 in wins and B >> 20 in wins
    top = big.site_summary(smc.ID_SPACE - 10, smc.ID_SPACE)
    assert len(top["n_rows"]) == 10 and not top["n_rows"].any()
    with pytest.raises(ValueError, match="not a range"):
        big.site_summary(smc.ID_SPACE - 1, smc.ID_SPACE + 1)
    big.site_summary_add(B + N, small.site_summary(0, 100), small.site_histogram(0, 100))
    assert np.array_equal(big.site_summary(B + N, B + N + 100)["n_rows"], want["summary"]["n_rows"][:100])
    small.close()
    big.close()


def test_11_switching(models, tickets):
    """dense -> sparse -> dense while a ticket is in flight: the ticket holds the table (and the map) it was submitted under; a
    budget smaller than the rows; the same arguments again zero nothing; the switch off"""
    tks = tickets
    al = Aligner(models["syn5"], "rna002", device=0)
    al.set_site_summary(NUM_SITES)
    al.set_site_histogram(*SPEC)
    t = submit(al, tks[0])
    al.set_site_summary(NUM_SITES, capacity=4096)                    # returns once the ticket is done
    s = al.site_summary()
    assert len(s["n_rows"]) == NUM_SITES and not any(c.any() for c in s["limbs"]) and not any(s["totals"].values())
    assert al.site_map() == {"capacity": 4096, "n_keys": 0, "rows_dropped": 0, "sites_dropped": 0}
    with pytest.raises(ValueError, match="set_site_histogram"):
        al.site_histogram()                                          # another mode released the histograms
    assert (t.wait().status == 0).all()
    t.close()
    t = submit(al, tks[1])
    al.set_site_summary(NUM_SITES, capacity=4096)                    # the same again: on, nothing zeroed, no wait needed
    t.wait()
    t.close()
    want = tks[1][2]                                                 # the dense table of the same ticket
    s = al.site_summary()
    assert all(bits(a) == bits(b) for a, b in zip(s["limbs"], want["limbs"])) and s["totals"] == want["totals"]
    assert al.site_map()["n_keys"] == int((want["n_rows"] > 0).sum())
    al.set_site_summary(0)                                           # off: the table and the map stay for the fetch
    with submit(al, tks[2]) as t3:
        t3.wait()
    assert bits(al.site_summary()["n_rows"]) == bits(want["n_rows"])
    al.set_site_summary(NUM_SITES, capacity=4096)
    t = submit(al, tks[2])
    al.set_site_summary(NUM_SITES)                                   # back to dense while a ticket is in flight
    with pytest.raises(ValueError, match="dense"):
        al.site_map()
    assert not al.site_summary()["n_rows"].any()
    t.wait()
    t.close()
    # a budget smaller than the rows: refused with rows and bytes; the handle is left without a table
    al.set_mem_budget(100000)
    with pytest.raises(MemoryError, match=r"sparse table of 4096 rows \(%d bytes\)" % (4096 * 60 + 64)):
        al.set_site_summary(NUM_SITES, capacity=4096)
    with pytest.raises(ValueError, match="capacity"):
        al.set_site_summary(NUM_SITES, capacity=0)
    al.close()


def test_11_switch_off_changes_nothing(models):
    """a sparse handle's job results are the bytes of a handle without the table"""
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    flat = np.concatenate(make_ids(reads, 8))
    al = Aligner(models["syn5"], "rna002", device=0)
    off = al.align_batch(sig, seq, True)
    al.set_site_summary(smc.ID_SPACE, capacity=1024)                 # too small for the reads' sites: rows are dropped, results are not
    on = al.align_batch(sig, seq, True, site_ids=flat)
    m = int(off.seg_offsets[-1])
    for col in ("Z", "status", "n_segments", "seg_offsets"):
        assert np.asarray(getattr(off, col)).tobytes() == np.asarray(getattr(on, col)).tobytes(), col
    for col in ("signal_positions", "sequence_positions", "probabilities", "states"):
        assert getattr(off, col)[:m].tobytes() == getattr(on, col)[:m].tobytes(), col
    st, t = al.site_map(), al.site_summary(0, 0)["totals"]
    assert st["n_keys"] <= 1024 and t["reads_ok"] == 48
    assert t["rows_added"] + t["rows_without_site"] + t["rows_skipped"] == m and t["rows_skipped"] >= st["rows_dropped"]
    al.close()
