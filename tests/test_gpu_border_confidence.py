"""GPU (-m gpu): per-border posterior confidence (Aligner.set_border_confidence, border_kernels.hpp). Whole reads through
every place a lattice lives -- the separate layout (plain and certified reads), the in-place layout, a page-starved pool, the
wide-band kernel -- against the NumPy restatement over the CPU oracle's lattices (tests/border_confidence_cases.py), within
the derived 1e-6; and the window sum itself, compiled into a test unit with the product's flags, on lattices the test writes:
out-of-band slots poisoned with 0.0 (mass 1 per cell), bit-equal to the same fp64 sum in NumPy.
Switching the columns on moves nothing else, and off is the launch it has always been."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import border_confidence_cases as bcc
from conftest import ROOT, model_for
from dynamont_amd import Aligner, _native, synth, zstd_io

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

COLS = ("border_probability", "border_window_probability")


# ---- shared: read sets and their yardsticks, computed once ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def sets(models):
    m = models["syn5"]
    return {
        "rna002": ("rna002", 400, bcc.plain_reads(m, "rna002", bcc.RNA002_SEED, 3, 120)),
        "dna_r9": ("dna_r9", 400, bcc.plain_reads(m, "dna_r9", bcc.DNA_R9_SEED, 3, 200)),
        "clipped": ("rna002", 400, bcc.plain_reads(m, "rna002", bcc.CLIPPED_SEED, 3, 60)),
        "band50": ("dna_r9", 50, bcc.imperfect_reads(m, "dna_r9", bcc.BAND50_SEED, 3, 200)),
        "band50_long": ("dna_r9", 50, bcc.imperfect_reads(m, "dna_r9", bcc.BAND50_LONG_SEED, 1, 600)),
        "wide": ("rna002", 600, bcc.plain_reads(m, "rna002", bcc.WIDE_SEED, 1, 600)),
    }


@pytest.fixture(scope="module")
def want(models, sets, oracle_built):
    """yardstick(set name, W) -> [(border_probability, border_window_probability, oracle result)] per read, cached"""
    from oracle.pyoracle import Oracle
    orcs, lpms, cache = {}, {}, {}

    def get(name, W):
        if (name, W) not in cache:
            pore, band, reads = sets[name]
            if (pore, band) not in orcs:
                orcs[pore, band] = Oracle(models["syn5"], synth.PORES[pore][0], band)
            out = []
            for i, r in enumerate(reads):
                if (name, i) not in lpms:                                  # the lattice once per read, whatever W
                    lpms[name, i] = bcc.lpm_columns(orcs[pore, band], r.signal, r.sequence, band)
                lpm, res = lpms[name, i]
                bp, bwp = bcc.from_lpm(lpm, res["signal_positions"].astype(np.int64) + 1, W)
                out.append((bp, bwp, res))
            cache[name, W] = out
        return cache[name, W]
    return get


def run(model, pore, band, reads, W, budget=None):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    al.set_border_confidence(W)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        b.align(True)
        res = b.fetch()
        tm = b.timing()
    al.close()
    return res, tm


def check(res, yard, what):
    """both columns of every read within TOL of the yardstick, along the oracle's own borders; returns the largest error"""
    worst = 0.0
    assert (res.status[:len(yard)] == 0).all(), (what, res.status)
    for i, (bp, bwp, orc_res) in enumerate(yard):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        assert m == len(bp) and np.array_equal(res.signal_positions[a:a + m], orc_res["signal_positions"]), (what, i)
        for got, ref, col in ((res.border_probability[a:a + m], bp, COLS[0]), (res.border_window_probability[a:a + m], bwp, COLS[1])):
            err = np.abs(got - ref)
            j = int(err.argmax())
            print(f"{what} read {i} {col}: max |got - yardstick| = {err[j]:.3e} at row {j} (got {got[j]!r}, want {ref[j]!r})")
            assert err[j] <= bcc.TOL, (what, i, col, j, got[j], ref[j])
            worst = max(worst, float(err[j]))
    return worst


def same_segments(a, b):
    """no segment, Z or probability moved"""
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "probabilities"):
        assert np.array_equal(getattr(a, col)[:m].view(np.uint64), getattr(b, col)[:m].view(np.uint64)), col


def run_off(model, pore, band, reads, budget=None):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    res = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
    assert res.border_probability is None and "border_probability" not in res.read(0)
    al.close()
    return res


# ---- 1. default layout, plain and certified reads ---------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 8])
@pytest.mark.parametrize("name", ["rna002", "dna_r9"])
def test_default_layout(models, sets, want, name, W):
    """rna002: pad + A, a structural tie at the read's start -- the launch that carries both arithmetic flavours, its strict
    branch; dna_r9: the plain launch. At W = 2 the yardstick spans 0.3 .. 1.0 on every rna002 read."""
    pore, band, reads = sets[name]
    yard = want(name, W)
    res, tm = run(models["syn5"], pore, band, reads, W)
    assert tm["lp_inplace"] == 0 and tm["launches"] == 1
    if name == "rna002":
        assert tm["reads_strict"] == len(reads)                     # every read carries the tie: the launch with both flavours
    else:
        assert tm["reads_strict"] == 0
    if name == "rna002" and W == 2:
        for _, bwp, _ in yard:
            assert bwp.min() <= 0.3 and bwp.max() >= 1.0 - bcc.TOL
    check(res, yard, f"{name} W={W}")
    d = res.read(1)
    a = int(res.seg_offsets[1])
    assert set(d) >= set(COLS) and np.array_equal(d[COLS[1]], res.border_window_probability[a:a + len(d[COLS[1]])])
    same_segments(res, run_off(models["syn5"], pore, band, reads))


# ---- 2. windows clipped at the read's ends ------------------------------------------------------------------------------------
def test_windows_clipped_at_the_reads_ends(models, sets, want):
    """3 rna002 reads of 60 bases, W = 64: 12-13 of each read's 56 windows reach past row 1 or T - 1"""
    pore, band, reads = sets["clipped"]
    yard = want("clipped", 64)
    for r, (bp, _, res) in zip(reads, yard):
        clipped, _ = bcc.window_counts(len(r.signal) + 1, len(r.sequence) - 5 + 2, band, res["signal_positions"].astype(np.int64) + 1, 64)
        assert 12 <= clipped <= 13 and len(bp) == 56
    res, _ = run(models["syn5"], pore, band, reads, 64)
    check(res, yard, "clipped W=64")


# ---- 3. windows that leave the band ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["band50", "band50_long"])
def test_windows_that_leave_the_band(models, sets, want, name):
    """dna_r9 imperfect reads at band = 50, W = 256. 200 bases: 92, 143 and 136 of the 196 / 201 / 196 windows hold out-of-band
    rows, and every value is 1. 600 bases: 593 lattice columns, so band slots wrap (a slot is n mod 448) and an unmasked read
    of a slot returns another column's value; 250 of the 592 windows leave the band."""
    pore, band, reads = sets[name]
    yard = want(name, 256)
    for r, (bp, bwp, res) in zip(reads, yard):
        N = len(r.sequence) - 5 + 2
        _, leaving = bcc.window_counts(len(r.signal) + 1, N, band, res["signal_positions"].astype(np.int64) + 1, 256)
        if name == "band50":
            assert 92 <= leaving <= 143 and np.abs(bwp - 1.0).max() <= bcc.TOL
        else:
            assert N > 448 and leaving == 250 and 4 * leaving >= len(bp)
    res, _ = run(models["syn5"], pore, band, reads, 256)
    check(res, yard, f"{name} W=256")
    if name == "band50":
        m = int(res.seg_offsets[-1])
        assert np.abs(res.border_window_probability[:m] - 1.0).max() <= 2 * bcc.TOL


# ---- 4. in-place layout and a page-starved pool ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["inplace", "page_starved"])
@pytest.mark.parametrize("name,W", [("rna002", 2), ("dna_r9", 8), ("band50", 256), ("band50_long", 256)])
def test_inplace_layout_and_page_starved_pool(models, sets, want, monkeypatch, name, W, path):
    pore, band, reads = sets[name]
    yard = want(name, W)
    budget = None
    if path == "page_starved" and name == "band50_long":
        # one read alone cannot queue for pages (and a budget of one and a half of its lattice refuses it): the long read
        # shares its batch, and its pool, with the three reads of 200 bases
        reads = sets["band50"][2] + reads
        yard = want("band50", W) + yard
    if path == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    else:
        # a read's lattice takes ~(448 * 8 + 56) bytes per row (tests/test_gpu_imperfect_reads.py sizes it so): room for a fifth
        # of the batch, and for the longest read one and a half times over
        lens = sorted((len(r.signal) for r in reads), reverse=True)
        budget = int(max(0.2 * sum(lens), 1.5 * lens[0]) * (448 * 8 + 56))
    res, tm = run(models["syn5"], pore, band, reads, W, budget)
    off = run_off(models["syn5"], pore, band, reads, budget)
    if path == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
        assert tm["lp_inplace"] == 1
        if name == "rna002":
            assert tm["reads_strict"] == len(reads)                 # in place AND both flavours: k_read_queue<JOB_ALIGN_INPLACE | JOB_BORDER, true>
        if name == "dna_r9":
            assert tm["reads_strict"] == 0                          # ... and the plain in-place launch
    else:
        print(f"{name} page-starved: pool_pages {tm['pool_pages']}, page_rows {tm['page_rows']}, n_static {tm['n_static']} of {len(reads)}")
    check(res, yard, f"{name} W={W} {path}")
    same_segments(res, off)


# ---- 5. wide band -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [8, 256])
def test_wide_band(models, sets, want, W):
    """one rna002 read of 600 bases at band = 600: half band 298, above the register sweeps' 223 -- the wide-band kernel (band_reads.hip)"""
    pore, band, reads = sets["wide"]
    assert min(band // 2, (len(reads[0].sequence) - 5 + 2) // 2) == 298
    res, _ = run(models["syn5"], pore, band, reads, W)
    check(res, want("wide", W), f"wide W={W}")
    same_segments(res, run_off(models["syn5"], pore, band, reads))


# ---- 6. the switch is per ticket and changes nothing else ----------------------------------------------------------------------
def test_switch_is_per_ticket_and_changes_nothing_else(models, oracle_built):
    from oracle.pyoracle import Oracle
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(7600 + j, 600, "rna004", mean, sd, (60, 120)) for j in range(2)]
    never = Aligner(models["syn9"], "rna004", device=0)                     # a handle that never switched it on
    base = [never.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads in data]
    never.close()
    al = Aligner(models["syn9"], "rna004", device=0)
    plan = [(0, 0), (2, 1), (8, 0), (0, 1), (2, 1)]                          # (W, data set), in submission order
    tickets = []
    for W, k in plan:
        al.set_border_confidence(W)
        tickets.append(al.align_async(*synth.pack_reads(data[k]), True))
    al.set_border_confidence(0)
    orc = Oracle(models["syn9"], synth.PORES["rna004"][0])
    cols = [np.zeros(int(base[0].cap) + int(base[1].cap)) for _ in range(2)]
    out = _native.DynBorderOut(*[c.ctypes.data_as(_native.c_double_p) for c in cols], len(cols[0]))
    results = []
    for (W, k), t in zip(plan, tickets):
        res = t.wait()
        results.append(res)
        same_segments(res, base[k])
        launches = t.timing()["launches"]
        if W == 0:
            assert res.border_probability is None
            assert launches == 0                                          # published into the resident session (600 reads)
            with pytest.raises(ValueError, match="without dyn_aligner_set_border_confidence"):
                t.fetch_borders(out)
        else:
            assert launches >= 1                                          # one launch per batch: no session for this ticket
            yard = []
            for r in data[k][:4]:
                bp, bwp, o = bcc.yardstick(orc, r.signal, r.sequence, W)
                yard.append((bp, bwp, o))
            check(res, yard, f"ticket W={W}")
            t.fetch_borders(out)
            m = int(res.seg_offsets[-1])
            assert np.array_equal(cols[1][:m].view(np.uint64), res.border_window_probability[:m].view(np.uint64))
    m = int(results[1].seg_offsets[-1])
    for c in COLS:                                                            # two runs of the same W > 0 ticket: the same bits
        assert np.array_equal(getattr(results[1], c)[:m].view(np.uint64), getattr(results[4], c)[:m].view(np.uint64)), c
    for t in tickets:
        t.close()
    st = al.session_stats()
    assert st["sessions"] >= 1 and st["aborted"] == 0                        # the W = 0 tickets between them opened one (again)
    al.close()


def test_fetch_fails_cleanly(models, sets):
    pore, band, reads = sets["dna_r9"]
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], pore, device=0)
    cols = [np.zeros(4096) for _ in range(2)]
    out = _native.DynBorderOut(*[c.ctypes.data_as(_native.c_double_p) for c in cols], 4096)
    with al.batch(sig, seq) as b:
        b.align(True)                          # switch off at submission
        al.set_border_confidence(5)
        with pytest.raises(ValueError, match="without dyn_aligner_set_border_confidence"):
            b.fetch_borders(out)
        b.align(False)                         # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_borders(out)
        b.align(True)
        b.fetch_borders(out)
        small = _native.DynBorderOut(*[c.ctypes.data_as(_native.c_double_p) for c in cols], 3)
        with pytest.raises(ValueError, match="capacity"):
            b.fetch_borders(small)
    al.close()


# ---- 7. together with the neighbours -------------------------------------------------------------------------------------------
def test_rescaling_values_are_the_last_passes(models, sets, oracle_built):
    from oracle.pyoracle import Oracle
    pore, band, reads = sets["dna_r9"]
    sig, seq = [np.ascontiguousarray(1.2 * r.signal + 0.3) for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], pore, device=0)
    al.set_rescale(1)
    al.set_border_confidence(8)
    with al.batch(sig, seq) as b:
        b.align(True)
        res = b.fetch()
        x = b.signals()
    al.close()
    off = np.concatenate([[0], np.cumsum([len(v) for v in sig])]).astype(np.int64)
    xs = [x[int(off[i]):int(off[i + 1])] for i in range(len(sig))]
    assert (res.status == 0).all() and (res.rescale_iters >= 1).all()
    assert all(not np.array_equal(a, s0) for a, s0 in zip(xs, sig))            # the signal the last pass aligned is not the input
    orc = Oracle(models["syn5"], synth.PORES[pore][0])
    check(res, [bcc.yardstick(orc, xs[i], seq[i], 8) for i in range(len(sig))], "rescale(1) W=8")


def test_all_three_opt_ins_on_one_batch_and_through_the_sink(models, sets, tmp_path):
    pore, band, reads = sets["dna_r9"]
    al = Aligner(models["syn5"], pore, device=0)
    L = _native.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    flags = _native.DYN_CSV_EVENT_STATS | _native.DYN_CSV_SEGMENT_SCORES | _native.DYN_CSV_BORDER_CONFIDENCE
    assert L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1,
                                  flags, C.byref(h), err, 1024) == 0, err.value
    sig, sig_off, seqs, seq_off = synth.pack_reads(reads)
    n = len(reads)
    rid = (C.c_char_p * n)(*[f"r{i}".encode() for i in range(n)])
    sid = (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)])
    starts = np.zeros(n, dtype=np.int64)
    lengths = np.diff(np.asarray(sig_off).astype(np.int64)).astype(np.uint64)
    so = np.ascontiguousarray(seq_off, dtype=np.uint64)

    def submit(t):
        return L.dyn_csv_sink_submit(h, al._h, t._h, C.byref(t.result._c), n, seqs, so.ctypes.data_as(_native.c_u64_p), rid, sid,
                                     starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(_native.c_u64_p))

    al.set_event_stats(True)
    al.set_segment_scores(8)
    lacking = al.align_async(sig, sig_off, seqs, seq_off, True)                # the two neighbours on, this switch off
    assert submit(lacking) == _native.DYN_ERR_INVALID_ARGUMENT and "DYN_CSV_BORDER_CONFIDENCE" in al.last_error()
    al.set_border_confidence(8)
    on = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(on) == 0
    assert L.dyn_csv_sink_wait(h, 1, -1) == 1
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    lines = zstd_io.decompress(open(tmp_path / "o.csv.zst", "rb").read()).split(b"\n")
    assert lines[0].endswith(b",polish,level_mean,level_stdv,level_median,median_delta,mad_delta,homogeneity,"
                             b"border_probability,border_window_probability")
    res = on.wait()
    for c in ("level_mean", "median_delta", "homogeneity") + COLS:
        assert getattr(res, c) is not None, c
    same_segments(res, lacking.wait())
    assert len(lines) - 2 == int(res.n_segments.sum())
    for j in (0, 1, int(res.n_segments[0]) - 1):
        want_tail = ",{:.6f},{:.6f},{:.6f},{:.6f},{:.6f},{:.6f},{:.6f},{:.6f}".format(
            *(getattr(res, c)[j] for c in ("level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity") + COLS))
        assert lines[1 + j].endswith(want_tail.encode()), (j, lines[1 + j], want_tail)
    lacking.close()
    on.close()
    al.close()


# ---- 8. the device harness ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("bconf") / "libbconf.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/border_confidence.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.bc_run.restype = C.c_int
    return lib


P_SLOTS, CPL = 448, 7
HALF_LOG_2PI = float.fromhex("0x1.d67f1c864beb4p-1")
FILL = 7.25        # what the harness's outputs hold where the kernel writes nothing


def row_pos(s):
    lane, j = s // CPL, s % CPL
    return (j >> 1) * 128 + lane * 2 + (j & 1) if j < 6 else 384 + lane


class Lattice:
    """a read of T rows and N columns (more than 448: slots wrap) with a narrow band, in all three layouts; every slot outside the
    band holds the poison 0.0 -- log-posterior 0, mass 1 -- and in-band cells random values, some -inf"""

    def __init__(self, seed=11, T=900, N=610, bw=20):
        rng = np.random.default_rng(seed)
        self.T, self.N, self.bw = T, N, bw
        self.ratio = N / T
        self.Zb, self.m1 = -1234.5678, float(np.log(0.07))
        self.rowmap = rng.permutation(T + 1).astype(np.uint32)              # lattice row t lives in row rowmap[t]: a page table
        B = 2 * bw + 3
        self.lp_in = np.zeros((T + 1, P_SLOTS, 2), dtype=np.float32)
        self.lp_wide = np.zeros((T, B, 2), dtype=np.float32)
        self.lpe = np.zeros((T + 1, P_SLOTS), dtype=np.float32)
        self.bE = np.zeros((T + 1, P_SLOTS))
        self.sig = rng.normal(0.0, 1.0, T - 1)
        mean, sd = rng.normal(0.0, 1.0, N - 1), rng.uniform(0.1, 0.4, N - 1)
        self.par = np.stack([mean, 1.0 / sd, -np.log(sd), sd], axis=1).copy()
        self.inband = np.zeros((T + 1, N + 1), dtype=bool)
        self.lpm = np.full((T + 1, N + 1), -np.inf)                          # what the in-place and wide accessors must return
        for t in range(1, T):
            start = int(t * self.ratio) - bw
            lo, hi = max(start, 1), min(start + 2 * bw + 1, N)
            for n in range(lo, hi):
                self.inband[t, n] = True
                v = np.float32(-np.inf) if rng.random() < 0.05 else np.float32(-rng.exponential(3.0))
                self.lpm[t, n] = float(v)
                pos = row_pos(n % P_SLOTS)
                self.lp_in[self.rowmap[t], pos] = (v, np.float32(-rng.exponential(3.0)))
                self.lp_wide[t, n - start + 1] = (v, np.float32(-rng.exponential(3.0)))
                dead = rng.random() < 0.03                                 # bE = -inf: nothing leaves the cell, so LPE = -inf too
                self.bE[self.rowmap[t], pos] = -np.inf if dead else -rng.exponential(5.0) - 1000.0
                self.lpe[self.rowmap[t], pos] = np.float32(-np.inf) if dead or rng.random() < 0.05 else np.float32(-rng.exponential(3.0))
        # borders: along the band's diagonal with a jitter, the first and the last row among them
        self.cols = np.array([1] + list(range(2, N - 1, 3)) + [N - 1], dtype=np.int32)
        rows = np.clip((self.cols / self.ratio).astype(np.int64) + rng.integers(-6, 7, len(self.cols)), 1, T - 1)
        rows[0], rows[-1] = 1, T - 1
        self.rows = rows.astype(np.int32)

    def emis(self, x, n):
        mean, inv, nls, _ = self.par[n - 1]
        z = (x - mean) * inv
        return (z * z * -0.5 + nls) - HALF_LOG_2PI        # fma(t, -0.5, nls): the product is exact, so this is the same rounding

    def separate(self, t, n):
        """BorderCellSeparate restated: LPM rebuilt from the float LPE and bE of (t-1, n-1), bE(t+1, n), two emissions, Zb, m1"""
        ib = self.inband
        if not ib[t, n] or t + 1 >= self.T or not ib[t + 1, n]:
            return -np.inf
        if t == 1:
            if n != 1:
                return -np.inf
            fE_prev = 0.0
        else:
            if not ib[t - 1, n - 1]:
                return -np.inf
            pos = row_pos((n - 1) % P_SLOTS)
            l = self.lpe[self.rowmap[t - 1], pos]
            if l == -np.inf:
                return -np.inf
            fE_prev = (float(l) - self.bE[self.rowmap[t - 1], pos]) + self.Zb
        fM = (fE_prev + self.emis(self.sig[t - 1], n)) + self.m1
        bM = self.bE[self.rowmap[t + 1], row_pos(n % P_SLOTS)] + self.emis(self.sig[t], n)
        return (fM + bM) - self.Zb

    def expected_lpm(self, layout, W):
        K = 2 * W + 1
        out = np.full((len(self.cols), K), FILL)
        for i, (n, r) in enumerate(zip(self.cols.tolist(), self.rows.tolist())):
            for k in range(K):
                t = r - W + k
                if 1 <= t <= self.T - 1:
                    out[i, k] = self.separate(t, n) if layout == 0 else self.lpm[t, n]
        return out


@pytest.fixture(scope="module")
def lattice():
    return Lattice()


@pytest.mark.parametrize("W", [1, 256])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_device_harness_window_sum(harness, lattice, layout, W):
    """border_kernels.hpp's accessors and window sum on a lattice of the test's own. Every accessor value equals the NumPy
    restatement bit for bit (so no poisoned slot was read: each would add mass 1); each term is that value's exponential; the
    sum is the terms added in ascending row order, bit for bit; borders in rows 1 and T - 1; W = 1 and 256."""
    la = lattice
    with np.errstate(invalid="ignore", over="ignore"):
        want_lpm = la.expected_lpm(layout, W)
    nb, K = want_lpm.shape
    lpm = np.full((nb, K), FILL)
    term = np.full((nb, K), FILL)
    here, total = np.full(nb, FILL), np.full(nb, FILL)
    err = np.full(64, -1, dtype=np.int32)
    lp = (la.lpe, la.lp_in, la.lp_wide)[layout]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = harness.bc_run(C.c_int(layout), C.c_int(la.T), C.c_int(la.N), C.c_int(la.bw), C.c_int(W), C.c_double(la.ratio),
                       C.c_double(la.Zb), C.c_double(la.m1), C.c_int(nb), p(la.cols), p(la.rows), C.c_uint64(la.rowmap.size),
                       p(la.rowmap), C.c_uint64(lp.size), p(lp), C.c_uint64(la.bE.size), p(la.bE), C.c_uint64(la.sig.size), p(la.sig),
                       C.c_uint64(la.par.shape[0]), p(la.par), p(lpm), p(term), p(here), p(total), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert not np.isnan(want_lpm).any()
    bad = np.argwhere(lpm.view(np.uint64) != want_lpm.view(np.uint64))
    assert bad.size == 0, (layout, W, bad[:5], lpm[tuple(bad[0])], want_lpm[tuple(bad[0])])
    inside = want_lpm != FILL
    finite = inside & np.isfinite(want_lpm)
    assert finite.sum() >= nb and (inside & ~finite).sum() >= (nb if W == 256 else 5)   # in-band values and masked cells, both
    assert (term[~inside] == FILL).all() and (term[inside & ~finite] == 0.0).all()
    ref = np.exp(want_lpm[finite])
    assert (np.abs(term[finite] - ref) <= 5e-16 * ref).all()                  # the device's exp: within two ulps of NumPy's
    for i in range(nb):
        s = 0.0
        for kk in range(K):
            if inside[i, kk]:
                s += term[i, kk]                                              # ascending row order, one IEEE add per term
        assert s.hex() == float(total[i]).hex(), (layout, W, i, s, total[i])
        assert float(here[i]).hex() == float(term[i, W]).hex()
    assert la.rows[0] == 1 and la.rows[-1] == la.T - 1 and (total > 0).sum() >= nb // 2
    if W == 256 and layout != 0:
        assert total.max() < 60.0     # a single unmasked row of poison would add 1 per cell: sums of ~500 rows stay near the band's width
