"""GPU (-m gpu): the two-sample comparison of the per-site histograms and the exact add (Aligner.site_compare,
Aligner.site_summary_add). Every output integer must EQUAL the restatement of the definition (tests/site_compare_cases.py):
  1. the product's comparison kernel on histograms the test uploads (tests/device_math/site_compare.hip, built with the product's
     flags), for 4, 8, 34, 66 and 256 counters per site: every group width, one, two and four rounds;
  2. the product's add kernel on a table, counters and columns the test uploads;
  3. whole reads through Aligner: two conditions in one table of 2 N sites, the restatement over site_histogram of both halves and
     over level_mean of the jobs' own event columns, the bound against the exact KS over those event means; the same bytes through
     a resident session and one launch per batch, and with the control saved, reset and added back; adds that double, that cross the
     staging step, that meet a ticket in flight; the new calls unused changing nothing.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import site_compare_cases as scc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth
from test_gpu_site_summary import make_ids, polya_reads

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

N = 3000                      # sites per sample: the table holds 2 N
SPEC = (32, -4.0, 4.0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("scomp") / "libscomp.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/site_compare.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.sc_run.restype = C.c_int
    lib.sa_run.restype = C.c_int
    return lib


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def assert_columns(got, want, what=""):
    for k in scc.COLUMNS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s %s: pairs %s device %s restatement %s" % (what, k, bad[:6].tolist(), g[bad[:6]].tolist(), w[bad[:6]].tolist())


# ---- 1. the device harness: comparison ---------------------------------------------------------------------------------------------
def run_compare(lib, table, w, site_lo, other_lo, count):
    out = np.full(10 * count, 0x5A5A5A5A, dtype=np.uint32)
    guard = np.array([0x1357246813572468], dtype=np.uint64)
    err = np.full(64, -1, dtype=np.int32)
    t = np.ascontiguousarray(table, dtype=np.uint32)
    k = lib.sc_run(C.c_uint32(t.shape[0]), C.c_int(w - 2), p(t), C.c_uint32(site_lo), C.c_uint32(other_lo), C.c_uint32(count), p(out),
                   p(guard), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert guard[0] == 0x1357246813572468                            # nothing written behind the output
    u64 = out[:4 * count].view(np.uint64)
    u32 = out[4 * count:]
    col = lambda i: u32[i * count:(i + 1) * count].copy()  # noqa: E731
    return dict(level_num=u64[:count].copy(), dwell_num=u64[count:].copy(), n_a=col(0), n_b=col(1), level_at=col(2), dwell_at=col(3),
                level_side=col(4).view(np.int32), dwell_side=col(5).view(np.int32)), out


@pytest.mark.parametrize("w", scc.WIDTHS)
def test_device_harness_compare(harness, w):
    """37 pairs (the last wave has dead lanes) per window; seeded random counts; a maximum in round 0; one in the last counter that
    can hold it, in the last round; a tie across rounds (the smaller index and ITS side win); equal sites; an empty A, an empty B,
    both; nA = nB = 2^32 - 1 at opposite ends. The other window below, a window overlapping itself by half, one pair starting at
    the table's last site, a window against itself. Poisoned output, a guard word behind it; twice, the same bits."""
    table = scc.compare_tables()[w]
    level, dwell = scc.split(table, w)
    for site_lo, other_lo, count in scc.WINDOWS:
        got, raw = run_compare(harness, table, w, site_lo, other_lo, count)
        assert_columns(got, scc.compare_arrays(level, dwell, site_lo, other_lo, count), "Bc %d window %s" % (w, (site_lo, other_lo, count)))
        assert np.array_equal(raw, run_compare(harness, table, w, site_lo, other_lo, count)[1])
    got, _ = run_compare(harness, table, w, *scc.WINDOWS[0])
    i = scc.BUILT.index("top")
    assert int(got["level_num"][i]) == (2 ** 32 - 1) ** 2 and got["level_at"][i] == 0 and got["level_side"][i] == 1
    i = scc.BUILT.index("tie")
    assert (got["level_at"][i], got["level_side"][i], got["dwell_at"][i], got["dwell_side"][i]) == (0, 1, 0, 1)
    i = scc.BUILT.index("last")
    assert got["level_at"][i] == w - 2 and got["dwell_at"][i] == 14 and got["level_side"][i] == -1
    same, _ = run_compare(harness, table, w, *scc.WINDOWS[3])
    assert not same["level_num"].any() and not same["dwell_num"].any() and not same["level_side"].any()


# ---- 2. the device harness: add ----------------------------------------------------------------------------------------------------
def run_add(lib, case, totals=True, hist_on=True, hist=None):
    acc = case["acc"].copy()
    hist = case["hist"].copy() if hist is None else hist.copy()
    err = np.full(64, -1, dtype=np.int32)
    cols, counters = np.ascontiguousarray(case["cols"]), np.ascontiguousarray(case["counters"])
    k = lib.sa_run(C.c_uint32(case["n_sites"]), C.c_int(scc.ADD_BINS), C.c_uint32(case["lo"]), C.c_uint32(len(cols)), p(cols),
                   p(case["totals"]) if totals else None, C.c_int(1 if hist_on else 0), p(counters), p(acc), p(hist), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    return acc, hist


@pytest.mark.parametrize("count", [1, 37])
def test_device_harness_add(harness, count):
    """a seeded table and counters; columns that force a carry from the low into the high limb of M1, a negative M2 increment, dwell_sq
    wrapping 2^64, a counter wrapping 2^32, a total wrapping 2^64. Totals given and NULL; histograms NULL leave a poisoned counter
    buffer untouched."""
    case = scc.add_case(count, 9100 + count)
    cols, counters = case["cols"].tolist(), case["counters"].tolist()
    s = case["lo"]
    want_acc, want_hist = scc.add_restated(case["acc"], case["hist"], case["n_sites"], scc.ADD_WIDTH, s, cols, case["totals"].tolist(), counters)
    assert int(want_acc[7 * s + 4]) == 7 and int(want_acc[7 * s + 2]) == 7                      # the carry; the wrap
    assert int(want_acc[7 * s + 6]) == 2 ** 64 - 1 and int(want_acc[7 * s + 5]) == 2 ** 64 - 11345
    assert int(want_hist[scc.ADD_WIDTH * s + 3]) == 0x10
    acc, hist = run_add(harness, case)
    assert np.array_equal(acc, want_acc), np.flatnonzero(acc != want_acc)[:8].tolist()
    assert np.array_equal(hist, want_hist), np.flatnonzero(hist != want_hist)[:8].tolist()
    want_acc, _ = scc.add_restated(case["acc"], case["hist"], case["n_sites"], scc.ADD_WIDTH, s, cols, None, None)
    poison = np.full_like(case["hist"], 0xA5A5A5A5)
    acc, hist = run_add(harness, case, totals=False, hist_on=False, hist=poison)
    assert np.array_equal(acc, want_acc) and (hist == 0xA5A5A5A5).all()
    assert np.array_equal(acc[-5:], case["acc"][-5:])


def test_device_harness_add_a_window_of_2_20_plus_3(harness):
    """more sites than one staging step of the product holds, in ONE launch here: columns that are zero except at 300 seeded rows,
    the first, the 2^20-th and the last; every other cell must come back as it went in"""
    n = (1 << 20) + 3
    rng = np.random.default_rng(77)
    acc = rng.integers(0, 1 << 62, 7 * n + 5, dtype=np.int64).astype(np.uint64)
    rows = sorted({0, (1 << 20) - 1, 1 << 20, n - 1} | set(rng.integers(0, n, 300).tolist()))
    cols = np.zeros((n, 7), dtype=np.uint64)
    cols[rows] = rng.integers(0, 1 << 63, (len(rows), 7), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    hist = np.full(n * scc.ADD_WIDTH, 0xA5A5A5A5, dtype=np.uint32)
    case = dict(n_sites=n, lo=0, acc=acc, hist=hist, cols=cols, counters=np.zeros(1, dtype=np.uint32), totals=np.arange(5, dtype=np.uint64))
    want, _ = scc.add_restated(acc, hist[:scc.ADD_WIDTH], n, scc.ADD_WIDTH, 0, cols, [0, 1, 2, 3, 4], None, rows=rows)
    got, h = run_add(harness, case, hist_on=False)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8].tolist()
    assert (h == 0xA5A5A5A5).all()


# ---- 3. whole reads ------------------------------------------------------------------------------------------------------------------
TRANSCRIPT, SHIFTED, SHIFT = 300, range(100, 110), 0.5


def two_conditions(models, n_reads=48):
    """two conditions of n_reads full-length reads each over ONE 300-base transcript (DNA: no pad); the second condition's samples of
    the bases 100 .. 109 are shifted by +0.5. ids: base b -> site b, the second condition offset by N."""
    _, mean, sd = synth.read_model_file(models["syn9"])
    k = 9
    mean_code, sd_code = synth.code_order_table(mean, sd, k, False)
    rng = np.random.default_rng(8800)
    digits = rng.integers(0, 4, TRANSCRIPT)
    seq = "".join("ACGT"[d] for d in digits)
    codes = synth._seq_codes(digits, k)
    out = []
    for cond in (0, 1):
        sig, ids = [], []
        for _ in range(n_reads):
            dw = np.maximum(2, rng.poisson(12.5, size=len(codes)))
            col = np.repeat(np.arange(len(codes)), dw)
            x = mean_code[codes[col]] + rng.uniform(0.8, 2.0) * sd_code[codes[col]] * rng.standard_normal(len(col))
            if cond:
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


def halves(al):
    h = al.site_histogram()
    return h["level"].tolist(), h["dwell"].tolist()


def compare_bytes(c):
    return b"".join(np.ascontiguousarray(c[k]).tobytes() for k in scc.COLUMNS)


def state_bytes(al):
    s, h = al.site_summary(), al.site_histogram()
    return b"".join(c.tobytes() for c in s["limbs"]) + repr(s["totals"]).encode() + h["level"].tobytes() + h["dwell"].tobytes()


def test_two_conditions_in_one_table(models):
    (sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b) = two_conditions(models)
    al = fresh(models)
    al.set_event_stats(True)
    res = [al.align_batch(sig, seq, True, site_ids=np.concatenate(ids)) for sig, seq, ids in ((sig_a, seq_a, ids_a), (sig_b, seq_b, ids_b))]
    assert all((r.status == 0).all() for r in res)
    got = al.site_compare(0, N)
    level, dwell = halves(al)
    assert_columns(got, scc.compare_arrays(level, dwell, 0, N, N), "site_histogram of both halves")
    assert compare_bytes(al.site_compare()) == compare_bytes(got) == compare_bytes(al.site_compare(0, N, N))
    win = al.site_compare(90, 130)
    assert all(np.array_equal(win[k], got[k][90:130]) for k in scc.COLUMNS)
    back = al.site_compare(N, 2 * N, 0)                               # the windows the other way round: the sides flip
    assert np.array_equal(back["level_num"], got["level_num"]) and np.array_equal(back["level_side"], -got["level_side"])
    assert np.array_equal(back["n_a"], got["n_b"])
    # level_mean of the jobs' own event columns, binned in NumPy with the definition's two operations
    half = al.kmer_size // 2
    per_site = [[[] for _ in range(N)] for _ in range(2)]
    for c, (r, ids) in enumerate(zip(res, (ids_a, ids_b))):
        for i in range(r.n):
            a, n = int(r.seg_offsets[i]), int(r.n_segments[i])
            for s, v in zip((ids[i][half:half + n].astype(np.int64) - c * N).tolist(), np.asarray(r.level_mean[a:a + n], dtype=np.float64).tolist()):
                per_site[c][s].append(v)
    mine = [[scc.binned(per_site[c][s], *SPEC) for s in range(N)] for c in range(2)]
    assert mine[0] == level[:N] and mine[1] == level[N:]
    covered = [s for s in range(N) if per_site[0][s] and per_site[1][s]]
    assert len(covered) == TRANSCRIPT - 2 * half and np.array_equal(np.flatnonzero(got["n_a"]), np.array(covered))
    assert (got["level_at"][got["n_a"] == 0] == scc.NO_AT).all() and np.isnan(got["level_d"][got["n_a"] == 0]).all()
    # section 1's bound against the exact KS over the raw event means, at every site
    for s in covered:
        num, den = scc.ks_exact(per_site[0][s], per_site[1][s])
        assert den == int(got["n_a"][s]) * int(got["n_b"][s])
        share = scc.bin_share(mine[0][s], mine[1][s])
        assert int(got["level_num"][s]) <= num and Fraction(num, den) <= Fraction(int(got["level_num"][s]), den) + share, (s, num, den, share)
        assert got["level_d"][s] == float(int(got["level_num"][s])) / (float(got["n_a"][s]) * float(got["n_b"][s]))
    at = got["level_at"][covered]
    edge = got["level_edge"][covered]
    assert np.array_equal(edge[at <= 32], SPEC[1] + at[at <= 32].astype(np.float64) * 0.25) and np.isinf(edge[at == 33]).all()
    # a sanity check only: the shifted bases stand out
    d = got["level_d"]
    far = [s for s in covered if s < SHIFTED[0] - 20 or s > SHIFTED[-1] + 20]
    assert np.median(d[list(SHIFTED)]) > np.median(d[far]), (np.median(d[list(SHIFTED)]), np.median(d[far]))
    # refusals
    with pytest.raises(ValueError, match=r"dyn_aligner_site_compare: the other window \[3001, 3001 \+ 3000\) does not end inside the table's 6000 sites"):
        al.site_compare(0, N, N + 1)
    with pytest.raises(ValueError, match=r"is not a range of the table's 6000 sites"):
        al.site_compare(0, 2 * N + 1, 0)
    assert al.site_compare(5, 5)["n_a"].size == 0
    al.close()


def test_session_and_launch_paths_and_a_control_added_back(models):
    """the same bytes: through a resident session and through one launch per batch; with the control aligned in the same process and
    with the control saved, reset and site_summary_add()ed back into [N, 2N). Adding the saved table twice doubles every integer."""
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
        got.append((compare_bytes(al.site_compare()), state_bytes(al)))
        if session:
            al.close()
    assert got[0] == got[1]
    # al: one launch per batch, both conditions in. Save the control half, start again, align the run, add the control back.
    saved, saved_h = al.site_summary(N, 2 * N), al.site_histogram(N, 2 * N)
    assert saved["n_rows"].sum() > 0
    al.reset_site_summary()
    al.align_batch(sig_a, seq_a, True, site_ids=np.concatenate(ids_a))
    run_totals = al.site_summary(0, 0)["totals"]
    ctl = dict(saved, totals={k: saved["totals"][k] - run_totals[k] for k in saved["totals"]})     # the control's own share
    al.site_summary_add(N, ctl, saved_h)
    assert (compare_bytes(al.site_compare()), state_bytes(al)) == got[1]
    # twice: every integer of the control's half doubles
    no_totals = {k: v for k, v in saved.items() if k != "totals"}
    al.site_summary_add(N, no_totals, saved_h)
    twice, twice_h = al.site_summary(N, 2 * N), al.site_histogram(N, 2 * N)
    assert all(np.array_equal(t, 2 * s) for t, s in zip(twice["limbs"][:3], saved["limbs"][:3]))
    assert [int(v) for v in twice["M1"]] == [2 * int(v) for v in saved["M1"]] and [int(v) for v in twice["M2"]] == [2 * int(v) for v in saved["M2"]]
    assert np.array_equal(twice_h["level"], 2 * saved_h["level"]) and np.array_equal(twice_h["dwell"], 2 * saved_h["dwell"])
    assert twice["totals"] == al.site_summary(0, 0)["totals"] and twice["totals"]["rows_added"] == saved["totals"]["rows_added"]
    # the table alone; refusals
    al.site_summary_add(N, no_totals)
    assert np.array_equal(al.site_summary(N, 2 * N)["n_rows"], 3 * saved["n_rows"]) and np.array_equal(al.site_histogram(N, 2 * N)["level"], twice_h["level"])
    wrong = dict(saved_h, edges=np.nextafter(saved_h["edges"], np.inf))
    with pytest.raises(ValueError, match="edges are not the handle's"):
        al.site_summary_add(N, no_totals, wrong)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_summary_add: \[3001, 6001\) is not a range of the table's 6000 sites"):
        al.site_summary_add(N + 1, no_totals)
    empty = {k: np.zeros(0, dtype=np.uint64) for k in ("n_rows", "n_samples", "dwell_sq")}
    before = state_bytes(al)
    al.site_summary_add(17, dict(empty, M1=[], M2=[], totals=[1, 2, 3, 4, 5]))                   # an empty window touches nothing
    assert state_bytes(al) == before
    al.close()
    plain = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    plain.set_site_summary(2 * N)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_summary_add: dyn_aligner_set_site_histogram\(a, bins > 0, lo, hi\) was never called on this handle"):
        plain.site_summary_add(N, no_totals, saved_h)
    with pytest.raises(ValueError, match=r"dyn_aligner_site_compare: dyn_aligner_set_site_histogram\(a, bins > 0, lo, hi\) was never called on this handle"):
        plain.site_compare(0, 10, 20)
    plain.site_summary_add(N, no_totals)                                                          # the table alone is fine
    assert np.array_equal(plain.site_summary(N, 2 * N)["n_rows"], saved["n_rows"])
    plain.close()


def test_add_across_the_staging_step(models):
    """a window of 2^20 + 3 sites into a table of that size: the right integers at the first, the 2^20-th and the last site"""
    n = (1 << 20) + 3
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    al.set_site_summary(n)
    cols = {k: np.zeros(n, dtype=np.uint64) for k in ("n_rows", "n_samples", "dwell_sq")}
    m1, m2 = np.zeros(n, dtype=object), np.zeros(n, dtype=object)
    marks = (0, (1 << 20) - 1, 1 << 20, n - 1)
    for j, s in enumerate(marks):
        cols["n_rows"][s], cols["n_samples"][s], cols["dwell_sq"][s] = 1 + j, 10 + j, (1 << 64) - 1 - j
        m1[s], m2[s] = -(1 << 70) - j, (1 << 100) + j
    for _ in range(2):
        al.site_summary_add(0, dict(cols, M1=m1, M2=m2, totals=[1, 2, 3, 4, 5]))
    for lo, hi in ((0, 500), ((1 << 20) - 500, n)):
        t = al.site_summary(lo, hi)
        assert t["totals"] == dict(reads_ok=2, rows_added=4, samples_added=6, rows_without_site=8, rows_skipped=10)
        assert (np.flatnonzero(t["n_rows"]) + lo).tolist() == [s for s in marks if lo <= s < hi]
        for j, s in enumerate(marks):
            if lo <= s < hi:
                assert (int(t["n_rows"][s - lo]), int(t["n_samples"][s - lo]), int(t["dwell_sq"][s - lo])) == (
                    2 + 2 * j, 20 + 2 * j, (2 * ((1 << 64) - 1 - j)) % (1 << 64))
                assert int(t["M1"][s - lo]) == 2 * (-(1 << 70) - j) and int(t["M2"][s - lo]) == 2 * ((1 << 100) + j)
    al.close()


def test_add_while_a_ticket_is_in_flight_loses_nothing(models):
    reads = polya_reads(models)
    idx = [i % 48 for i in range(512)]
    ids48 = make_ids(reads, 10)
    packed, flat = synth.pack_reads([reads[i] for i in idx]), np.concatenate([ids48[i] for i in idx])
    al = fresh(models, sites=N, session=True, pore="rna002", model="syn5")
    with al.align_async(*packed, True, site_ids=flat) as t:
        t.wait()
    once, once_h = al.site_summary(), al.site_histogram()
    assert once["n_rows"].sum() > 10000
    al.reset_site_summary()
    t = al.align_async(*packed, True, site_ids=flat)
    al.site_summary_add(0, once, once_h)                              # while the ticket may still be adding
    assert (t.wait().status == 0).all()
    t.close()
    both, both_h = al.site_summary(), al.site_histogram()
    assert all(np.array_equal(b, 2 * o) for b, o in zip(both["limbs"][:3], once["limbs"][:3]))
    assert [int(v) for v in both["M1"]] == [2 * int(v) for v in once["M1"]] and [int(v) for v in both["M2"]] == [2 * int(v) for v in once["M2"]]
    assert np.array_equal(both_h["level"], 2 * once_h["level"]) and np.array_equal(both_h["dwell"], 2 * once_h["dwell"])
    assert both["totals"] == {k: 2 * v for k, v in once["totals"].items()}
    al.close()


def test_the_new_calls_unused_change_nothing(models):
    """site_summary / site_histogram / site_quantiles of the same reads: the same bytes on a handle that compared and added (into
    other sites) as on one that never did"""
    reads = polya_reads(models)
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    flat = np.concatenate(make_ids(reads, 8))
    got = []
    for use in (False, True):
        al = fresh(models, sites=N, pore="rna002", model="syn5")
        if use:
            al.site_compare(0, 100, 200)
            al.site_summary_add(N - 1, dict(n_rows=[0], n_samples=[0], dwell_sq=[0], M1=[0], M2=[0]))
        res = al.align_batch(sig, seq, True, site_ids=flat)
        if use:
            al.site_compare(0, N // 2)
        q = al.site_quantiles([0.25, 0.5, 0.75])
        got.append((state_bytes(al), b"".join(q[k].tobytes() for k in ("n", "rank", "bin", "below", "in_bin")), res.signal_positions.tobytes()))
        al.close()
    assert got[0] == got[1]
