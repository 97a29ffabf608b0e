"""GPU (-m gpu): the per-read site calls (Aligner.set_site_calls, Aligner.set_site_model). Every double of the two columns must EQUAL,
by its bits, the restatement of the definition in Python floats (tests/site_call_cases.py):
  1. the product's kernels on arrays the test uploads (tests/device_math/site_calls.hip, built with the product's flags): one read
     with rows of 1, 255, 256, 257 and 16 385 + 64 samples (the short / long split, the wrap of the chunk loop), a read of only short
     rows in the same launch, a failed read and a read outside [read_lo, read_hi) whose rows keep the poison; ids without a site,
     outside the table, with an unset, a one-component and a two-component model row; event means that drive the exp argument past
     -512 and -1 024; q_0 == q_1; an event mean whose square reaches 2^64. Dense, and sparse with a map so small that the last
     uploaded id finds its probe window full: that id has no call, the call kernels leave n_keys alone, and the upload inserts set
     rows only. A poisoned output with a guard word behind it; twice, the same bytes.
  2. whole reads through Aligner: the two conditions of tests/test_gpu_site_mixture.py, site_mixture, set_site_model, then the
     reads again with set_site_calls and set_event_stats: the restatement over level_mean, the ids and site_model(); one launch per
     batch, merged tickets and the resident session; sparse at load 0.5 against dense; the 2^20 staging step of the upload; the
     argument errors and refusals; the switch off changing nothing; and, at the shifted sites, more called rows among the
     shifted reads than among the others.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import site_call_cases as scc
import site_summary_cases as ssc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from test_gpu_site_mixture import N, SHIFTED, SPEC, TRANSCRIPT, two_conditions

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

POISON = np.array([0x5A5A5A5A5A5A5A5A], dtype=np.uint64).view(np.float64)[0]
GUARD = 0x1357246813572468
K = 9                                         # syn9: output row j is base j + K // 2


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("scall") / "libscall.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_calls.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.sc_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def batch():
    return scc.build_batch()


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def same_bits(got, want, what):
    bad = np.flatnonzero(scc.bits(got) != scc.bits(want))
    assert bad.size == 0, (what, bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


# ---- 1. the device harness -----------------------------------------------------------------------------------------------------------
def run_calls(lib, b, read_lo, read_hi, capacity=0, windows=scc.WINDOWS):
    n_seg = b.segrow.size
    out = np.full(2 * n_seg, POISON, dtype=np.float64)
    guard = np.array([GUARD], dtype=np.uint64)
    err = np.full(96, -1, dtype=np.int32)
    keys = np.zeros(max(1, capacity), dtype=np.uint32)
    counts = np.zeros(3, dtype=np.uint64)
    lo = np.array([w[0] for w in windows], dtype=np.uint32)
    cnt = np.array([w[1] for w in windows], dtype=np.uint32)
    rows = np.ascontiguousarray(np.concatenate([scc.model_rows(*w) for w in windows])) if windows else np.zeros((1, 5))
    k = lib.sc_run(C.c_int(b.read.size), p(b.sig_off), p(b.par_off), p(b.seg_off), p(b.T), p(b.N), p(b.read), C.c_int(b.status.size), p(b.status),
                   C.c_uint64(b.sig.size), p(b.sig), C.c_uint64(n_seg), p(b.segrow), C.c_uint64(b.sites.size), p(b.sites),
                   C.c_uint32(scc.NUM_SITES), C.c_uint32(capacity), C.c_int(len(windows)), p(lo), p(cnt), p(rows), C.c_uint32(read_lo),
                   C.c_uint32(read_hi), p(out), p(guard), p(keys), p(counts), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert guard[0] == GUARD                                             # nothing written behind the output
    return out[:n_seg].copy(), out[n_seg:].copy(), keys, counts, out


def test_device_harness_dense(harness, batch):
    """three read ranges, each twice: the same bytes, and every double the restatement's; rows of the failed read and of the reads
    outside the range keep the poison"""
    b = batch
    n = len(b.reads)
    for lo, hi in ((scc.READ_LO, scc.READ_HI), (scc.OUTSIDE + 1, n), (0, n)):
        prob, z, _, _, raw = run_calls(harness, b, lo, hi)
        want_p, want_z = scc.reference(b.reads, scc.MODEL, scc.NUM_SITES, lo, hi, poison=POISON)
        same_bits(prob, want_p, "site_probability, reads [%d, %d)" % (lo, hi))
        same_bits(z, want_z, "site_z, reads [%d, %d)" % (lo, hi))
        assert raw.tobytes() == run_calls(harness, b, lo, hi)[4].tobytes()
        kept = np.isin(b.row_read, [i for i, (st, _) in enumerate(b.reads) if st != 0 or not lo <= i < hi])
        assert kept.any() and (scc.bits(prob[kept]) == scc.bits([POISON])[0]).all() and (scc.bits(z[kept]) == scc.bits([POISON])[0]).all()
        assert not (scc.bits(prob[~kept]) == scc.bits([POISON])[0]).any()     # every other row was written
    # no model rows at all: every row of the range is the NaN
    prob, z, _, _, _ = run_calls(harness, b, 0, n, windows=())
    live = np.isin(b.row_read, [i for i, (st, _) in enumerate(b.reads) if st == 0])
    assert (scc.bits(prob[live]) == scc.NAN_BITS).all() and (scc.bits(z[live]) == scc.NAN_BITS).all()


def test_device_harness_sparse(harness, batch):
    """a map of 8 buckets: the first window's 8 set rows fill it (its unset row inserts nothing), the second window's set row finds
    no bucket and is counted; the call kernels find, never insert"""
    b = batch
    n = len(b.reads)
    prob, z, keys, counts, raw = run_calls(harness, b, 0, n, capacity=scc.CAPACITY)
    present = set(int(k) for k in keys if k != scc.NONE)
    assert present == set(scc.SET_FIRST) and len(keys) == scc.CAPACITY
    assert counts.tolist() == [scc.CAPACITY, scc.CAPACITY, 1]            # n_keys after the uploads, after the calls; set rows dropped
    want_p, want_z = scc.reference(b.reads, scc.MODEL, scc.NUM_SITES, 0, n, present=present, poison=POISON)
    same_bits(prob, want_p, "site_probability, sparse")
    same_bits(z, want_z, "site_z, sparse")
    late = b.sites == scc.LATE
    assert late.sum() >= 3 and (scc.bits(prob[late]) == scc.NAN_BITS).all() and (scc.bits(z[late]) == scc.NAN_BITS).all()
    assert raw.tobytes() == run_calls(harness, b, 0, n, capacity=scc.CAPACITY)[4].tobytes()
    # a map with room: the dense bytes, and only set rows hold a key
    prob2, z2, keys2, counts2, _ = run_calls(harness, b, 0, n, capacity=64)
    dense = run_calls(harness, b, 0, n)
    assert prob2.tobytes() == dense[0].tobytes() and z2.tobytes() == dense[1].tobytes()
    assert set(int(k) for k in keys2 if k != scc.NONE) == set(scc.SET_FIRST) | {scc.LATE} and counts2.tolist() == [9, 9, 0]


# ---- 2. whole reads ------------------------------------------------------------------------------------------------------------------
def fresh(models, capacity=None, session=None, sites=2 * N):
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    if session is not None:
        al.set_session_mode(session)
    al.set_site_summary(sites, capacity=capacity)
    al.set_site_histogram(*SPEC)
    return al


def restate(res, ids, model, lo=0):
    """the two columns of a result from its level_mean, the reads' per-base ids and the model rows of [lo, lo + len)"""
    prob = np.zeros(res.cap)
    z = np.zeros(res.cap)
    rows = np.stack([model[k] for k in scc.COLUMNS], axis=1)
    for i in range(res.n):
        if res.status[i] != 0:
            continue
        a, nseg = int(res.seg_offsets[i]), int(res.n_segments[i])
        for j, s in enumerate(ssc.row_ids(ids[i], nseg, K)):
            row = rows[s - lo] if s != scc.NONE and lo <= s < lo + len(rows) else None
            prob[a + j], z[a + j] = (scc.NAN, scc.NAN) if row is None else scc.call(tuple(row), float(res.level_mean[a + j]))
    return prob, z


def per_read(res, attr):
    return [getattr(res, attr)[int(res.seg_offsets[i]):int(res.seg_offsets[i]) + int(res.n_segments[i])].tobytes() for i in range(res.n)]


@pytest.fixture(scope="module")
def fitted(models):
    """both conditions aligned into one table of 2 N sites, the pooled mixture of every site pair, and -- with that model uploaded
    for both halves -- the second condition's reads again with the calls and the levels on"""
    (sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b) = two_conditions(models)
    al = fresh(models)
    for sig, seq, ids in ((sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b)):
        assert (al.align_batch(sig, seq, True, site_ids=np.concatenate(ids)).status == 0).all()
    m = al.site_mixture(0, N, N)
    up = [al.set_site_model(0, m), al.set_site_model(N, m)]
    model = al.site_model()
    al.set_site_calls(True)
    al.set_event_stats(True)
    res_b = al.align_batch(sig_b, seq_b, True, site_ids=np.concatenate(ids_b))
    res_a = al.align_batch(sig_a, seq_a, True, site_ids=np.concatenate(ids_a))
    al.close()
    return dict(m=m, up=up, model=model, a=(sig_a, seq_a, ids_a, res_a), b=(sig_b, seq_b, ids_b, res_b))


def test_calls_equal_the_restatement_and_separate_the_shifted_reads(fitted):
    m, model = fitted["m"], fitted["model"]
    keep = np.isin(m["status"], (0, 2))
    assert fitted["up"] == [{"stored": int(keep.sum()), "dropped": 0}] * 2 and keep.sum() > 150
    for k in scc.COLUMNS:                                              # m["pi1"] etc. went through unchanged; every other row is unset
        want = np.where(keep, m[k], 0.0)
        assert model[k][:N].tobytes() == want.tobytes() and model[k][N:].tobytes() == want.tobytes(), k
    for cond in ("a", "b"):
        sig, seq, ids, res = fitted[cond]
        assert (res.status == 0).all() and res.site_probability.dtype == np.float64 and res.site_probability.shape == (res.cap,)
        want_p, want_z = restate(res, ids, model)
        same_bits(res.site_probability, want_p, "site_probability, condition " + cond)
        same_bits(res.site_z, want_z, "site_z, condition " + cond)
        d = res.read(5)
        a = int(res.seg_offsets[5])
        assert d["site_probability"].tobytes() == res.site_probability[a:a + len(d["site_z"])].tobytes() and len(d["site_z"]) == int(res.n_segments[5])
    # the ordering: at the shifted sites the shifted reads (two of three of the second condition) hold more called rows than the others
    sig, seq, ids, res = fitted["b"]
    called = {True: [], False: []}
    for i in range(res.n):
        a, nseg = int(res.seg_offsets[i]), int(res.n_segments[i])
        row_site = np.array(ssc.row_ids(ids[i], nseg, K)) - N
        at = np.isin(row_site, list(SHIFTED))
        with np.errstate(invalid="ignore"):
            called[i % 3 != 0] += (res.site_probability[a:a + nseg][at] >= 0.5).tolist()
    share = {k: float(np.mean(v)) for k, v in called.items()}
    print("share of rows called at the shifted sites: shifted reads %.3f, the others %.3f (%d / %d rows)" %
          (share[True], share[False], len(called[True]), len(called[False])))
    assert len(called[True]) == 320 and len(called[False]) == 160 and share[True] > share[False]


def test_the_same_bytes_on_every_launch_path(models, fitted):
    """one launch per batch, the resident session (a ticket of 528 reads) and four tickets queued behind a busy one (merged launches):
    every read's two columns are the bytes the synchronous batch gave it"""
    sig, seq, ids, res = fitted["b"]
    want = {c: per_read(res, c) for c in ("site_probability", "site_z", "level_mean")}
    reads = [synth.SynthRead(x, s) for x, s in zip(sig, seq)]
    idx = [i % 24 for i in range(528)]
    big = (synth.pack_reads([reads[i] for i in idx]), np.concatenate([ids[i] for i in idx]))
    parts = [(synth.pack_reads([reads[i] for i in idx[j:j + 132]]), np.concatenate([ids[i] for i in idx[j:j + 132]]), idx[j:j + 132])
             for j in range(0, 528, 132)]

    def handle(session):
        al = fresh(models, session=session)
        al.set_site_model(0, fitted["m"])
        al.set_site_model(N, fitted["m"])
        al.set_site_calls(True)
        al.set_event_stats(True)
        return al

    def check(got, which, what):
        for c in want:
            mine = per_read(got, c)
            assert [mine[r] == want[c][i] for r, i in enumerate(which)] == [True] * len(which), (what, c)

    for session in (True, False):
        al = handle(session)
        with al.align_async(*big[0], True, site_ids=big[1]) as t:
            got = t.wait()
            assert t.timing()["launches"] == (0 if session else 1)
        check(got, idx, "session %s" % session)
        al.close()
    al = handle(False)
    al.set_auto_guide(0)
    merged = False
    for attempt in range(3):     # (whether tickets meet in the queue is a matter of timing, as in tests/test_gpu_site_summary.py)
        ahead = al.align_async(*big[0], True, site_ids=big[1])
        ts = [al.align_async(*pk, True, site_ids=flat) for pk, flat, _ in parts]
        ahead.wait()
        ahead.close()
        for t, (_, _, which) in zip(ts, parts):
            check(t.wait(), which, "merged, attempt %d" % attempt)
            merged |= t.timing()["launch_share"] < 1.0
            t.close()
        if merged:
            break
    assert merged
    al.close()


def test_sparse_at_load_one_half_equals_dense(models, fitted):
    """the model's set rows and the rows of the job take their buckets in a map of twice as many rows as the 2 * 300 ids in play"""
    sig, seq, ids, res = fitted["b"]
    al = fresh(models, capacity=4 * TRANSCRIPT)
    up = [al.set_site_model(0, fitted["m"]), al.set_site_model(N, fitted["m"])]
    assert up == fitted["up"]
    keys_before = al.site_map()["n_keys"]
    assert keys_before == 2 * up[0]["stored"]                          # set rows only
    got_model = al.site_model()
    assert all(got_model[k].tobytes() == fitted["model"][k].tobytes() for k in scc.COLUMNS)
    al.set_site_calls(True)
    al.set_event_stats(True)
    got = al.align_batch(sig, seq, True, site_ids=np.concatenate(ids))
    st = al.site_map()
    assert st["rows_dropped"] == 0 and st["n_keys"] <= 2 * TRANSCRIPT and st["n_keys"] * 2 <= st["capacity"]
    for c in ("site_probability", "site_z", "level_mean"):
        assert getattr(got, c).tobytes() == getattr(res, c).tobytes(), c
    # a map too small for the model: the dropped rows are counted, and their sites have no call
    al.close()
    small = fresh(models, capacity=64)
    up = small.set_site_model(0, fitted["m"])
    assert up["stored"] == fitted["up"][0]["stored"] and up["dropped"] == up["stored"] - small.site_map()["n_keys"] > 0
    small.reset_site_model()
    assert not any(small.site_model(0, N)[k].any() for k in scc.COLUMNS)
    small.close()


def test_across_the_staging_step_of_the_upload(models):
    """a model of 2^20 + 3 sites uploaded in one call: set rows around the 2^20-th site, read back as sent; and the reads' ids mapped
    onto those sites score against them"""
    n = (1 << 20) + 3
    marks = [0, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, n - 1]
    m = {k: np.zeros(n) for k in scc.COLUMNS}
    rng = np.random.default_rng(31)
    for s in marks:
        mu = rng.uniform(-1, 1)
        for k, v in zip(scc.COLUMNS, (rng.uniform(0.2, 0.8), mu, mu + 0.6, rng.uniform(0.02, 0.3), rng.uniform(0.02, 0.3))):
            m[k][s] = v
    (sig, seq, ids), _ = two_conditions(models, 6)
    ids = [np.array([marks[int(b) % len(marks)] if b % 7 else b for b in v], dtype=np.uint32) for v in ids]   # (b % 7 == 0: an unset site)
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    al.set_site_summary(n)
    assert al.set_site_model(0, m) == {"stored": len(marks), "dropped": 0}
    back = al.site_model()
    assert all(back[k].tobytes() == m[k].tobytes() for k in scc.COLUMNS)
    al.set_site_calls(True)
    al.set_event_stats(True)
    res = al.align_batch(sig, seq, True, site_ids=np.concatenate(ids))
    al.close()
    want_p, want_z = restate(res, ids, m)
    same_bits(res.site_probability, want_p, "site_probability")
    same_bits(res.site_z, want_z, "site_z")
    assert np.isfinite(res.site_probability).sum() > 1000 and np.isnan(res.site_z).sum() > 100


def test_argument_errors_and_refusals(models, fitted):
    sig, seq, ids, _ = fitted["b"]
    sig, seq, flat = sig[:4], seq[:4], np.concatenate(ids[:4])
    m = {k: fitted["m"][k][:10] for k in scc.COLUMNS}
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_model: dyn_aligner_set_site_summary\(a, num_sites > 0\) was never called on this handle"):
        al.set_site_model(0, m)
    al.set_site_calls(True)
    with pytest.raises(ValueError, match=r"dyn_batch_align: dyn_aligner_set_site_calls is on, which needs dyn_aligner_set_site_summary\(a, num_sites > 0\)"):
        al.align_batch(sig, seq, True)
    with pytest.raises(ValueError, match=r"dyn_batch_align_async: dyn_aligner_set_site_calls is on, which needs dyn_aligner_set_site_summary"):
        al.align_async(*synth.pack_reads([synth.SynthRead(x, s) for x, s in zip(sig, seq)]), True)
    al.set_site_summary(100)
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_calls is on, which scores the rows of align\(calc_probabilities = 1\) jobs alone"):
        al.align_batch(sig, seq, False)
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_calls is on, which scores the rows of align\(calc_probabilities = 1\) jobs alone"):
        al.train_batch(sig, seq)
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_model: \[95, 105\) is not a range of the table's 100 sites"):
        al.set_site_model(95, m)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_model_fetch: \[0, 101\) is not a range of the table's 100 sites"):
        al.site_model(0, 101)
    assert al.set_site_model(100, {k: np.zeros(0) for k in scc.COLUMNS}) == {"stored": 0, "dropped": 0}
    assert not al.site_model()["var0"].any()                          # never uploaded: no row is set
    # asked, but no ids staged / no model uploaded: NaN columns
    for site_ids in (None, flat % 100):
        res = al.align_batch(sig, seq, True, site_ids=site_ids)
        rows = int(res.seg_offsets[-1])
        assert (scc.bits(res.site_probability[:rows]) == scc.NAN_BITS).all() and (scc.bits(res.site_z[:rows]) == scc.NAN_BITS).all()
    al.set_site_summary(0)
    with pytest.raises(ValueError, match=r"dyn_aligner_set_site_model: dyn_aligner_set_site_summary\(a, num_sites > 0\) is off on this handle"):
        al.set_site_model(0, m)
    al.set_site_summary(100)
    al.set_mem_budget(100 * 56 + 5 * 8 + 100)
    with pytest.raises(MemoryError, match=r"dyn_aligner_set_site_model: the site model of 100 sites \(4000 bytes\) does not fit dyn_aligner_set_mem_budget's"):
        al.set_site_model(0, m)
    al.close()


def test_the_switch_off_changes_nothing(models, fitted):
    """the same reads on a handle that never heard of the calls, on one with a model but the switch off, and on one with the switch
    on: every other output's bytes are the same, and only the last result carries the two columns"""
    sig, seq, ids, _ = fitted["b"]
    flat = np.concatenate(ids)
    got = []
    for use in (0, 1, 2):
        al = fresh(models)
        al.set_event_stats(True)
        al.set_segment_scores(4)
        if use:
            al.set_site_model(N, fitted["m"])
        al.set_site_calls(use == 2)
        res = al.align_batch(sig, seq, True, site_ids=flat)
        assert (res.site_probability is None) == (use < 2) and (res.site_z is None) == (use < 2)
        assert ("site_z" in res.read(0)) == (use == 2)
        s, h = al.site_summary(), al.site_histogram()
        rows = int(res.seg_offsets[-1])
        got.append(b"".join(np.ascontiguousarray(getattr(res, c)[:rows] if getattr(res, c).shape[0] == res.cap else getattr(res, c)).tobytes()
                            for c in ("Z", "status", "n_segments", "seg_offsets", "signal_positions", "sequence_positions", "probabilities", "states",
                                      "level_mean", "level_stdv", "level_median", "median_delta", "mad_delta", "homogeneity")) +
                   b"".join(c.tobytes() for c in s["limbs"]) + repr(s["totals"]).encode() + h["level"].tobytes() + h["dwell"].tobytes())
        al.close()
    assert got[0] == got[1] == got[2]
