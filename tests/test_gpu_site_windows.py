"""GPU (-m gpu): every window call of the per-site table across its 2^20 staging step, in ONE call over the whole window: the add
with counters and totals, site_summary, site_histogram, site_quantiles, site_compare (and site_mixture on the sparse table). The
step is where a call's offsets into the caller's columns, its staging slots sized for the largest window and the "totals once,
with the first window" rule live (tests/test_gpu_site_mixture.py and tests/test_gpu_site_compare.py cross it for site_mixture and
for an add without counters).
A table of n + 3 sites, n = 2^20 + 3, is empty but for six marked sites on both sides of the step and at the table's end; the
pair calls run over n pairs at a distance of 3 sites, so two pairs hold marks on both sides (2^20 - 1 with 2^20 + 2 -- either
side of the step --, 2^20 + 2 with the table's last site). At the marks the results equal the restatements
(tests/site_histogram_cases.py, tests/site_compare_cases.py) of the doubled input, everywhere else what they give for an empty
site. A sparse table of 64 rows returns the same bytes.
No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import numpy as np
import pytest

import site_compare_cases as scc
import site_histogram_cases as shc
import site_mixture_cases as smc
from dynamont_amd import Aligner

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

STEP = 1 << 20
N = STEP + 3                  # pairs of the pair calls; the table holds N + 3 sites
SPEC = (6, -3.0, 3.0)         # bins of width 1: inv_w is exact
MARKS = (0, STEP - 1, STEP, STEP + 1, N - 1, N + 2)
TOTALS = [1, 2, 3, 4, 5]
BC = SPEC[0] + 2


def marked_input():
    """the add's arguments: cells whose limbs use all 128 bits and counters at the marks, zeros everywhere else"""
    rng = np.random.default_rng(616)
    cols = {k: np.zeros(N + 3, dtype=np.uint64) for k in ("n_rows", "n_samples", "dwell_sq")}
    m1, m2 = np.zeros(N + 3, dtype=object), np.zeros(N + 3, dtype=object)
    level, dwell = np.zeros((N + 3, BC), dtype=np.uint32), np.zeros((N + 3, scc.DWELL_BINS), dtype=np.uint32)
    for j, s in enumerate(MARKS):
        cols["n_rows"][s], cols["n_samples"][s], cols["dwell_sq"][s] = 1 + j, 10 + j, (1 << 64) - 1 - j
        m1[s], m2[s] = -(1 << 70) - j, (1 << 100) + j
        level[s] = smc.two_condition(rng, *SPEC, 150, 150, 0.4, 0.2, 0.04)[j % 2]
        dwell[s] = rng.integers(0, 50, scc.DWELL_BINS)
    return dict(cols, M1=m1, M2=m2, totals=TOTALS), level, dwell


def run(models, capacity):
    """the same two adds and the same reads on a dense (capacity None) or a sparse table"""
    summary, level, dwell = marked_input()
    al = Aligner(models["syn9"], "dna_r10_400bps", device=0)
    al.set_site_summary(N + 3, capacity)
    al.set_site_histogram(*SPEC)
    hist = dict(level=level, dwell=dwell, edges=al.site_histogram(0, 0)["edges"])
    for _ in range(2):
        al.site_summary_add(0, summary, hist)
    out = dict(summary=al.site_summary(0, N + 3), histogram=al.site_histogram(0, N + 3), quantiles=al.site_quantiles(shc.PROBS, 0, N + 3),
               compare=al.site_compare(0, N, 3), mixture=al.site_mixture(0, N, 3), map=al.site_map() if capacity else None)
    al.close()
    return out, level, dwell


@pytest.fixture(scope="module")
def dense(models):
    return run(models, None)


def rest_of(n, live):
    rest = np.ones(n, dtype=bool)
    rest[list(live)] = False
    return rest


def test_dense_calls_across_the_staging_step(dense):
    got, level, dwell = dense
    t = got["summary"]
    assert t["totals"] == dict(reads_ok=2, rows_added=4, samples_added=6, rows_without_site=8, rows_skipped=10)  # once per call
    rest = rest_of(N + 3, MARKS)
    assert not any(limb[rest].any() for limb in t["limbs"])
    for j, s in enumerate(MARKS):
        assert (int(t["n_rows"][s]), int(t["n_samples"][s]), int(t["dwell_sq"][s])) == (2 + 2 * j, 20 + 2 * j, (2 * ((1 << 64) - 1 - j)) % (1 << 64))
        assert int(t["M1"][s]) == 2 * (-(1 << 70) - j) and int(t["M2"][s]) == 2 * ((1 << 100) + j)

    h = got["histogram"]
    assert np.array_equal(h["level"], 2 * level) and np.array_equal(h["dwell"], 2 * dwell)
    assert level[list(MARKS)].any(axis=1).all() and not level[rest].any() and not dwell[rest].any()

    q = got["quantiles"]
    names = ("rank", "bin", "below", "in_bin")
    want_n, want = shc.quantile_arrays((2 * level[list(MARKS)]).tolist(), shc.PROBS)
    assert np.array_equal(q["n"][list(MARKS)], want_n) and (want_n == 300).all()
    assert all(np.array_equal(q[k][list(MARKS)], w) for k, w in zip(names, want))
    zero_n, zero = shc.quantile_arrays([[0] * BC], shc.PROBS)
    assert not q["n"][rest].any() and zero_n[0] == 0
    assert all((q[k][rest] == w[0]).all() for k, w in zip(names, zero))

    c = got["compare"]
    live = sorted({s for s in MARKS if s < N} | {s - 3 for s in MARKS if 0 <= s - 3 < N})
    both = [s for s in live if s in MARKS and s + 3 in MARKS]
    assert both == [STEP - 1, N - 1]
    rows = [scc.compare_pair((2 * level[s]).tolist(), (2 * dwell[s]).tolist(), (2 * level[s + 3]).tolist(), (2 * dwell[s + 3]).tolist()) for s in live]
    assert all(r["n_a"] == 300 and r["n_b"] == 300 and r["level_num"] > 0 for r, s in zip(rows, live) if s in both)
    empty = scc.compare_pair([0] * BC, [0] * scc.DWELL_BINS, [0] * BC, [0] * scc.DWELL_BINS)
    rest = rest_of(N, live)
    for k in scc.COLUMNS:
        assert c[k].dtype == scc.DTYPES[k] and c[k].shape == (N,)
        assert np.array_equal(c[k][live], np.array([r[k] for r in rows], dtype=scc.DTYPES[k])), k
        assert (c[k][rest] == np.array(empty[k], dtype=scc.DTYPES[k])).all(), k


def test_sparse_table_returns_the_same_bytes(models, dense):
    want = dense[0]
    got = run(models, 64)[0]
    assert got["map"] == dict(capacity=64, n_keys=len(MARKS), rows_dropped=0, sites_dropped=0)
    assert got["summary"]["totals"] == want["summary"]["totals"]
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got["summary"]["limbs"], want["summary"]["limbs"]))
    for call, keys in (("histogram", ("level", "dwell")), ("quantiles", ("n", "rank", "bin", "below", "in_bin")), ("compare", scc.COLUMNS),
                       ("mixture", smc.COLUMNS)):
        for k in keys:
            g, w = got[call][k], want[call][k]
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (call, k)
