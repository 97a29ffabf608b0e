"""GPU (-m gpu): the per-site two-component mixture fit (Aligner.site_mixture). Every output -- the seven doubles by their bit
patterns, the six counts -- must EQUAL the restatement of the definition in Python floats (tests/site_mixture_cases.py):
  1. the product's kernel on tables the test uploads (tests/device_math/site_mixture.hip, built with the product's flags), for 8,
     18, 34, 66, 130 and 256 counters per site: group widths 8, 32 and 64, one to four rounds; 37 pairs per window (the last wave
     has dead lanes); the other window below the first, a window overlapping itself by half, one pair at the table's last site, a
     window against itself, the single-sample form; built sites (tests/site_mixture_cases.py, BUILT) beside seeded random ones;
  2. whole reads through Aligner: two conditions in one table of 2 N sites, the restatement over site_histogram of both halves; the
     same bytes through a resident session and one launch per batch, and across the 2^20 staging step; argument errors; the new
     call unused changing nothing.
Wrong versions these cases tell from the definition (tests/test_site_mixture_host.py asserts that the built sites do, for those
the restatement can express):
  - a reduction that crosses the group border: groups of 8 and 32 lanes share a wave with neighbours of other counts, and the same
    site meets other neighbours in another window (the sites 40 .. 57 are A in window 0 and B in window 1; the window against
    itself and the single-sample form shift every group by other amounts);
  - a finished group that keeps updating: "fast" (a handful of rounds) sits next to "slow" (runs to max_iters) in one wave, and
    "crossing" moves on after it has converged;
  - under / over inside the fit: "outside_only", "outliers";
  - a pooled count that wraps: "top" (2^32 - 1 rows on either side);
  - shares from the g of the round before the last M-step: "slow", "collapse", "crossing";
  - labels exchanged in the parameters but not in the shares: "crossing".
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import site_mixture_cases as smc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from test_gpu_site_summary import make_ids, polya_reads

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

N = 3000                      # sites per sample: the table holds 2 N
SPEC = (32, -4.0, 4.0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("smix") / "libsmix.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_mixture.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.sm_run.restype = C.c_int
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def assert_columns(got, want, what=""):
    bad = smc.same_bits(got, want)
    assert bad is None, (what,) + bad


# ---- 1. the device harness -----------------------------------------------------------------------------------------------------------
def run_mixture(lib, table, w, site_lo, other_lo, count, max_iters, tol, min_n):
    out = np.full(20 * count, 0x5A5A5A5A, dtype=np.uint32)
    guard = np.array([0x1357246813572468], dtype=np.uint64)
    err = np.full(64, -1, dtype=np.int32)
    t = np.ascontiguousarray(table, dtype=np.uint32)
    k = lib.sm_run(C.c_uint32(t.shape[0]), C.c_int(w - 2), p(t), C.c_uint32(site_lo), C.c_uint32(0xFFFFFFFF if other_lo is None else other_lo),
                   C.c_uint32(count), C.c_double(smc.H_LO), C.c_double(smc.H_HI), C.c_uint32(max_iters), C.c_double(tol), C.c_uint32(min_n),
                   p(out), p(guard), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert guard[0] == 0x1357246813572468                            # nothing written behind the output
    f64 = out[:14 * count].view(np.float64)
    u32 = out[14 * count:]
    got = {c: f64[i * count:(i + 1) * count].copy() for i, c in enumerate(smc.DOUBLES)}
    got.update({c: u32[i * count:(i + 1) * count].copy() for i, c in enumerate(smc.COUNTS)})
    return got, out


@pytest.mark.parametrize("w", smc.WIDTHS)
def test_device_harness_mixture(harness, w):
    """every window of site_mixture_cases.WINDOWS at max_iters = 24, the first one again at max_iters = 1; poisoned output, a guard
    word behind it; twice, the same bytes"""
    table = smc.mixture_tables()[w]
    level = smc.level_of(table, w)
    spec = smc.spec_of(w)
    for site_lo, other_lo, count in smc.WINDOWS:
        got, raw = run_mixture(harness, table, w, site_lo, other_lo, count, **smc.H_PARAMS)
        want = smc.fit_arrays(level, site_lo, other_lo, count, spec, key=w, **smc.H_PARAMS)
        assert_columns(got, want, "Bc %d window %s" % (w, (site_lo, other_lo, count)))
        assert np.array_equal(raw, run_mixture(harness, table, w, site_lo, other_lo, count, **smc.H_PARAMS)[1])
    once = dict(smc.H_PARAMS, max_iters=1)
    got1, _ = run_mixture(harness, table, w, *smc.WINDOWS[0], **once)
    assert_columns(got1, smc.fit_arrays(level, *smc.WINDOWS[0], spec, key=w, **once), "Bc %d max_iters 1" % w)
    assert int(got1["iters"].max()) == 1
    # what the built sites are (tests/test_site_mixture_host.py holds the restatement to the same)
    got, _ = run_mixture(harness, table, w, *smc.WINDOWS[0], **smc.H_PARAMS)
    st = {k: (int(got["status"][i]), int(got["iters"][i])) for i, k in enumerate(smc.BUILT)}
    assert st["fast"][0] == 0 and st["fast"][1] <= 6 and st["slow"] == (2, smc.H_PARAMS["max_iters"]) and st["collapse"][0] == 3, st
    assert all(st[k] == (1, 0) for k in ("empty_both", "one_bin", "below_min_n", "outside_only")) and st["at_min_n"][0] == 0
    i = smc.BUILT.index("one_bin")
    assert all(np.isnan(got[c][i]) for c in smc.DOUBLES) and (got["n_a"][i], got["n_b"][i]) == (30, 12)
    i = smc.BUILT.index("top")
    assert got["n_a"][i] == got["n_b"][i] == smc.M32 and got["r_b"][i] > 4.29e9 and got["status"][i] == 0
    assert (got["mu1"][got["status"] != 1] >= got["mu0"][got["status"] != 1]).all()


# ---- 2. whole reads ------------------------------------------------------------------------------------------------------------------
TRANSCRIPT, SHIFTED, SHIFT = 300, range(100, 110), 0.5
CHECKED = ((0, 6), (84, 126), (286, 300))        # windows of run sites the restatement is formed for: uncovered, shifted, the end


def two_conditions(models, n_reads=48):
    """two conditions of n_reads full-length reads each over ONE 300-base transcript (DNA: no pad), as tests/test_gpu_site_compare.py
    builds its own; in the second condition the samples of the bases 100 .. 109 are shifted by +0.5 in TWO reads of three. ids:
    base b -> site b, the second condition offset by N."""
    _, mean, sd = synth.read_model_file(models["syn9"])
    k = 9
    mean_code, sd_code = synth.code_order_table(mean, sd, k, False)
    rng = np.random.default_rng(8810)
    digits = rng.integers(0, 4, TRANSCRIPT)
    seq = "".join("ACGT"[d] for d in digits)
    codes = synth._seq_codes(digits, k)
    out = []
    for cond in (0, 1):
        sig, ids = [], []
        for i in range(n_reads):
            dw = np.maximum(2, rng.poisson(12.5, size=len(codes)))
            col = np.repeat(np.arange(len(codes)), dw)
            x = mean_code[codes[col]] + rng.uniform(0.8, 2.0) * sd_code[codes[col]] * rng.standard_normal(len(col))
            if cond and i % 3:
                x = x + SHIFT * np.isin(col + k // 2, list(SHIFTED))          # output row j is base j + k / 2
            sig.append(np.ascontiguousarray(x, dtype=np.float64))
            ids.append((cond * N + np.arange(TRANSCRIPT)).astype(np.uint32))
        out.append((sig, [seq] * n_reads, ids))
    return out


def fresh(models, sites=2 * N, session=None, pore="dna_r10_400bps", model="syn9"):
    al = Aligner(models[model], pore, device=0)
    if session is not None:
        al.set_session_mode(session)
    al.set_site_summary(sites)
    al.set_site_histogram(*SPEC)
    return al


def mixture_bytes(m):
    return b"".join(np.ascontiguousarray(m[k]).tobytes() for k in smc.COLUMNS)


def state_bytes(al):
    s, h = al.site_summary(), al.site_histogram()
    return b"".join(c.tobytes() for c in s["limbs"]) + repr(s["totals"]).encode() + h["level"].tobytes() + h["dwell"].tobytes()


def test_two_conditions_in_one_table(models):
    (sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b) = two_conditions(models)
    al = fresh(models)
    for sig, seq, ids in ((sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b)):
        assert (al.align_batch(sig, seq, True, site_ids=np.concatenate(ids)).status == 0).all()
    got = al.site_mixture(0, N, N)
    alone = al.site_mixture(0, N)
    level = al.site_histogram()["level"].tolist()
    for lo, hi in CHECKED:
        win = {k: got[k][lo:hi] for k in smc.COLUMNS}
        assert_columns(win, smc.fit_arrays(level, lo, N + lo, hi - lo, SPEC, **smc.DEFAULTS), "site_histogram of both halves [%d, %d)" % (lo, hi))
        assert_columns({k: alone[k][lo:hi] for k in smc.COLUMNS}, smc.fit_arrays(level, lo, None, hi - lo, SPEC, **smc.DEFAULTS), "the run alone")
        assert mixture_bytes(al.site_mixture(lo, hi, N + lo)) == mixture_bytes(win)                       # a window is a slice
    assert mixture_bytes(al.site_mixture(0, N, N, max_iters=128, tol=1e-3, min_n=8)) == mixture_bytes(got)  # the defaults
    few = al.site_mixture(84, 126, N + 84, max_iters=3, tol=0.0, min_n=2)
    assert_columns(few, smc.fit_arrays(level, 84, N + 84, 42, SPEC, max_iters=3, tol=0.0, min_n=2), "other parameters")
    assert np.isin(few["status"], (1, 2)).all() and (few["iters"][few["status"] == 2] == 3).all() and (few["status"] == 2).sum() > 20
    back = al.site_mixture(N, 2 * N, 0)                               # the windows the other way round: the same pooled fit
    assert np.array_equal(back["n_a"], got["n_b"]) and np.array_equal(back["out_b"], got["out_a"])
    for k in ("pi1", "mu0", "mu1", "var0", "var1", "iters", "status"):
        assert back[k].tobytes() == got[k].tobytes(), k               # (a + b == b + a; r_a and r_b change places)
    assert back["r_a"].tobytes() == got["r_b"].tobytes() and back["r_b"].tobytes() == got["r_a"].tobytes()
    # the host's columns
    fit = got["status"] != 1
    assert fit.sum() > 150 and np.isnan(got["pi1"][~fit]).all() and (got["iters"][~fit] == 0).all()
    assert np.array_equal(got["sd0"][fit], np.sqrt(got["var0"][fit])) and np.array_equal(got["sd1"][fit], np.sqrt(got["var1"][fit]))
    both = fit & (got["n_a"] > 0) & (got["n_b"] > 0)
    assert np.array_equal(got["share_a"][both], got["r_a"][both] / got["n_a"][both].astype(np.float64))
    assert np.array_equal(got["share_b"][both], got["r_b"][both] / got["n_b"][both].astype(np.float64))
    assert np.array_equal(got["separation"][fit], (got["mu1"][fit] - got["mu0"][fit]) / np.sqrt(0.5 * (got["var0"][fit] + got["var1"][fit])))
    assert np.isnan(got["share_a"][got["n_a"] == 0]).all() and np.isnan(alone["share_b"]).all() and not alone["n_b"].any()
    # a sanity check only: at the shifted bases the control... the second sample holds more of the upper component than the first
    delta = got["share_b"] - got["share_a"]
    far = [s for s in np.flatnonzero(both).tolist() if s < SHIFTED[0] - 20 or s > SHIFTED[-1] + 20]
    print("share_b - share_a: shifted", delta[list(SHIFTED)].tolist(), "median elsewhere", np.nanmedian(delta[far]), "fitted", int(fit.sum()))
    assert np.nanmedian(delta[list(SHIFTED)]) > 0.25 > abs(np.nanmedian(delta[far])), (np.nanmedian(delta[list(SHIFTED)]), np.nanmedian(delta[far]))
    # refusals
    with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: the other window \[3001, 3001 \+ 3000\) does not end inside the table's 6000 sites"):
        al.site_mixture(0, N, N + 1)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: \[0, 6001\) is not a range of the table's 6000 sites"):
        al.site_mixture(0, 2 * N + 1)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: max_iters 0 is not 1 \.\. 1024"):
        al.site_mixture(0, N, N, max_iters=0)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: max_iters 1025 is not 1 \.\. 1024"):
        al.site_mixture(0, N, N, max_iters=1025)
    for tol in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: tol must be finite and >= 0"):
            al.site_mixture(0, N, N, tol=tol)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: min_n 1 is not >= 2"):
        al.site_mixture(0, N, N, min_n=1)
    assert al.site_mixture(5, 5, 9)["status"].size == 0 and al.site_mixture(7, 7)["pi1"].size == 0
    al.close()
    plain = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    plain.set_site_summary(2 * N)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_mixture: dyn_aligner_set_site_histogram\(a, bins > 0, lo, hi\) was never called on this handle"):
        plain.site_mixture(0, 10, 20)
    plain.close()


def test_session_and_launch_paths(models):
    """the same bytes through a resident session and through one launch per batch"""
    rep = lambda v: [v[i % 24] for i in range(528)]  # noqa: E731  (a session is opened for a ticket of 512 reads or more)
    (sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b) = [tuple(rep(v) for v in cond) for cond in two_conditions(models, 24)]
    got = []
    for session in (True, False):
        al = fresh(models, session=session)
        for sig, seq, ids in ((sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b)):
            reads = [synth.SynthRead(x, s) for x, s in zip(sig, seq)]
            with al.align_async(*synth.pack_reads(reads), True, site_ids=np.concatenate(ids)) as t:
                assert (t.wait().status == 0).all()
                assert t.timing()["launches"] == (0 if session else 1)
        m = al.site_mixture(0, N, N)
        got.append((mixture_bytes(m), mixture_bytes(al.site_mixture(0, 2 * N)), state_bytes(al)))
        al.close()
    assert got[0] == got[1]
    assert (m["status"] != 1).sum() > 150


def test_across_the_staging_step(models):
    """a window of 2^20 + 3 pairs: the marked sites around the 2^20-th pair hold counters, every other site is empty. The single-sample
    form over the whole table and the two-window form at a distance of 3 sites equal the restatement at the marks and are 'no fit'
    everywhere else."""
    n = (1 << 20) + 3
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    al.set_site_summary(n + 3)
    al.set_site_histogram(*SPEC)
    edges = al.site_histogram(0, 0)["edges"]
    rng = np.random.default_rng(515)
    marks = (0, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, n - 1, n + 2)
    rows = {}
    for s in marks:
        a, b = smc.two_condition(rng, *SPEC, 150, 150, 0.4, 0.2, 0.04)
        rows[s] = [u + v for u, v in zip(a, b)]
        zero = np.zeros(1, dtype=np.uint64)
        al.site_summary_add(s, dict(n_rows=zero, n_samples=zero, dwell_sq=zero, M1=[0], M2=[0]),
                            dict(level=np.array([rows[s]], dtype=np.uint32), dwell=np.zeros((1, 16), dtype=np.uint32), edges=edges))
    empty = [0] * (SPEC[0] + 2)
    got = al.site_mixture(0, n)
    two = al.site_mixture(0, n, 3)
    al.close()
    for m, other in ((got, None), (two, 3)):
        live = sorted({s for s in marks if s < n} | ({s - 3 for s in marks if 0 <= s - 3 < n} if other else set()))
        want = [smc.fit(rows.get(s, empty), None if other is None else rows.get(s + other, empty), *SPEC, **smc.DEFAULTS) for s in live]
        want = {c: np.array([r[c] for r in want], dtype=np.float64 if c in smc.DOUBLES else np.uint32) for c in smc.COLUMNS}
        assert_columns({c: m[c][live] for c in smc.COLUMNS}, want, "marks, other %s" % other)
        assert (want["status"] == 0).all()
        rest = np.ones(n, dtype=bool)
        rest[live] = False
        assert (m["status"][rest] == 1).all() and np.isnan(m["mu0"][rest]).all() and not m["n_a"][rest].any() and not m["iters"][rest].any()
        assert all((m[c][rest].view(np.uint64) == 0x7FF8000000000000).all() for c in smc.DOUBLES)


def test_the_new_call_unused_changes_nothing(models):
    """site_summary / site_histogram / site_quantiles / site_compare of the same reads: the same bytes on a handle that fitted
    mixtures (before and after the reads) as on one that never did"""
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    flat = np.concatenate(make_ids(reads, 8))
    got = []
    for use in (False, True):
        al = fresh(models, sites=N, pore="rna002", model="syn5")
        if use:
            al.site_mixture(0, 100, 200)
        res = al.align_batch(sig, seq, True, site_ids=flat)
        if use:
            al.site_mixture(0, N // 2, N // 2)
            al.site_mixture()
        q = al.site_quantiles([0.25, 0.5, 0.75])
        c = al.site_compare(0, N // 2)
        got.append((state_bytes(al), b"".join(q[k].tobytes() for k in ("n", "rank", "bin", "below", "in_bin")),
                    b"".join(np.ascontiguousarray(c[k]).tobytes() for k in sorted(c)), res.signal_positions.tobytes()))
        al.close()
    assert got[0] == got[1]
