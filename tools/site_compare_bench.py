#!/usr/bin/env python
"""GPU box: what the two-sample comparison on the device (Aligner.site_compare) saves over the host route. One table of 2 x 2^20
sites with histograms (bins = 32 over [-4, 4)), both halves filled with seeded counters through Aligner.site_summary_add (timed as
well). Two wall times over ONE window of 2^20 pairs, best of 3, each after its own warm-up:
  device   Aligner.site_compare(0, 2^20): the kernel, 40 bytes per pair back, the host's two divisions
  host     two site_histogram() fetches of 2^20 sites each plus NumPy: cumulative sums, the two products, |x - y|, argmax
and whether the two give the same integers. Prints one JSON line and writes it to argv[1] if given
(profiles/site_compare/cost.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dynamont_amd import Aligner, synth

N = 1 << 20
BINS, LO, HI = 32, -4.0, 4.0
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
al = Aligner(model, "rna004", device=0)
al.set_site_summary(2 * N)
al.set_site_histogram(BINS, LO, HI)
rng = np.random.default_rng(12)
edges = LO + np.arange(BINS + 1, dtype=np.float64) * ((HI - LO) / BINS)
t_add = []
for half in range(2):
    # a site's rows spread over a few neighbouring bins around a centre of its own, as event means do; one site in 16 empty
    centre = rng.integers(4, BINS - 4, N)
    level = np.zeros((N, BINS + 2), dtype=np.uint32)
    for k in range(-3, 4):
        level[np.arange(N), centre + k] = rng.integers(0, 40, N) // (1 + abs(k))
    level[rng.random(N) < 1 / 16] = 0
    dwell = np.zeros((N, 16), dtype=np.uint32)
    dwell[:, 2:6] = (level.sum(axis=1)[:, None] // 4).astype(np.uint32)
    rows = level.sum(axis=1).astype(np.uint64)
    zeros = np.zeros(N, dtype=object)
    t0 = time.perf_counter()
    al.site_summary_add(half * N, {"n_rows": rows, "n_samples": rows * np.uint64(10), "dwell_sq": rows * np.uint64(100), "M1": zeros, "M2": zeros},
                        {"level": level, "dwell": dwell, "edges": edges})
    t_add.append(time.perf_counter() - t0)


def host_route():
    t0 = time.perf_counter()
    a, b = al.site_histogram(0, N)["level"], al.site_histogram(N, 2 * N)["level"]
    t_fetch = time.perf_counter() - t0
    pa, pb = np.cumsum(a, axis=1, dtype=np.uint64), np.cumsum(b, axis=1, dtype=np.uint64)
    na, nb = pa[:, -1], pb[:, -1]
    x, y = pa * nb[:, None], pb * na[:, None]
    dist = np.where(x > y, x - y, y - x)
    at = np.argmax(dist, axis=1)                                    # the first maximum: the smallest index
    num = dist[np.arange(N), at]
    side = np.sign(x[np.arange(N), at].astype(np.int64) - y[np.arange(N), at].astype(np.int64)).astype(np.int32)   # (counts far below 2^31)
    empty = (na == 0) | (nb == 0)
    return (na.astype(np.uint32), nb.astype(np.uint32), np.where(empty, 0, num), np.where(empty, 0xFFFFFFFF, at).astype(np.uint32),
            np.where(empty, 0, side).astype(np.int32)), time.perf_counter() - t0, t_fetch


al.site_compare(0, N)                                               # warm-up: the staging buffer, the kernel's first launch
t_dev = []
for _ in range(3):
    t0 = time.perf_counter()
    got = al.site_compare(0, N)
    t_dev.append(time.perf_counter() - t0)
host_route()                                                        # warm-up
t_host, t_fetch = [], []
for _ in range(3):
    want, t, tf = host_route()
    t_host.append(t)
    t_fetch.append(tf)
same = all(np.array_equal(g, w) for g, w in zip((got["n_a"], got["n_b"], got["level_num"], got["level_at"], got["level_side"]), want))
al.close()
rec = {"window_pairs": N, "bins": BINS, "table_sites": 2 * N, "covered_pairs": int(((got["n_a"] > 0) & (got["n_b"] > 0)).sum()),
       "device_ms_best_of_3": round(1e3 * min(t_dev), 3), "device_ms": [round(1e3 * t, 3) for t in t_dev],
       "host_ms_best_of_3": round(1e3 * min(t_host), 3), "host_ms": [round(1e3 * t, 3) for t in t_host],
       "of_which_two_fetches_ms": round(1e3 * min(t_fetch), 3), "ratio_host_over_device": round(min(t_host) / min(t_dev), 2),
       "same_integers": bool(same), "site_summary_add_ms_per_2_20_sites_with_counters": [round(1e3 * t, 1) for t in t_add],
       "bytes_back_per_pair": {"device": 40, "host": 2 * 4 * (BINS + 18)}}
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
