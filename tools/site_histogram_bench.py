#!/usr/bin/env python
"""GPU box: what the per-site histograms (Aligner.set_site_histogram) cost on the async align line, and what the quantile kernel
saves. After tools/site_summary_bench.py: cfg2's shape (1 024 reads x ~20 k samples, syn9, band 400) through align_async in steady
state (DEPTH tickets in flight), THREE settings alternating in ONE process, each after its own warm-up, REPS times, medians:
`off`, `summary` (the per-site table alone) and `hist` (the table and the histograms, bins = 32 over [-4, 4)). Two id patterns:
`uniform` over 10^8 sites (a 5.6 GB table and 20 GB of counters) and `hot`, every read on one 2 000-site transcript (1 024 adds per
batch on a handful of 4-byte counters that share cache lines within a site). The yardstick is the `summary` line of the same
process. Per pattern also: dyn_aligner_site_quantiles over one window of 2^20 sites (or the whole table when it is smaller)
against site_histogram() of the same window scanned in NumPy (cumsum + argmax per probability), wall time, best of 3.
Prints one JSON line and writes it to argv[1] if given (profiles/site_histogram/cost.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("SH_BATCHES", 12))
WARMUP = int(os.environ.get("SH_WARMUP", 4))
REPS = int(os.environ.get("SH_REPS", 3))
DEPTH = int(os.environ.get("SH_DEPTH", 4))
PATTERNS = {"uniform": 100_000_000, "hot": 2_000}
BINS, LO, HI = 32, -4.0, 4.0
SETTINGS = ("off", "summary", "hist")
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"])) for j in range(2)]
samples = [int(p[1][-1]) for p in packed]


def make_ids(seq_off, num_sites, rng):
    lens = np.diff(seq_off.astype(np.int64))
    out = np.empty(int(seq_off[-1]), dtype=np.uint32)
    for i, n in enumerate(lens.tolist()):
        start = 0 if num_sites <= n else int(rng.integers(0, num_sites - n))
        out[int(seq_off[i]):int(seq_off[i]) + n] = (start + np.arange(n)) % num_sites
    return out


def measure(name, num_sites):
    rng = np.random.default_rng(11)
    ids = [make_ids(p[3], num_sites, rng) for p in packed]
    al = Aligner(model, cfg["pore"], band=400, device=0)
    al.set_site_summary(num_sites)
    al.set_site_histogram(BINS, LO, HI)                 # allocated once: the settings below only flip the switches

    def run(setting, n):
        """n batches under `setting`, DEPTH in flight; wall time from the first submit to the last wait"""
        al.set_site_summary(0 if setting == "off" else num_sites)
        if setting == "hist":
            al.set_site_histogram(BINS, LO, HI)
        else:
            al.set_site_histogram(0)
        t0 = time.perf_counter()
        inflight, done, seg_ms, resident = [], 0, [], 0

        def finish(t, k):
            nonlocal done, resident
            t.wait()
            tm = t.timing()
            seg_ms.append(tm["ms_total"] - tm["ms_dp"])
            resident += tm["launches"] == 0
            t.close()
            done += samples[k]

        for j in range(n):
            inflight.append((al.align_async(*packed[j % 2], True, site_ids=None if setting == "off" else ids[j % 2]), j % 2))
            if len(inflight) >= DEPTH:
                finish(*inflight.pop(0))
        for t, k in inflight:
            finish(t, k)
        return done / (time.perf_counter() - t0) / 1e6, seg_ms, resident

    rate = {s: [] for s in SETTINGS}
    ms = {s: [] for s in SETTINGS}
    res = dict.fromkeys(SETTINGS, 0)
    for r in range(REPS):
        for setting in SETTINGS[r % 3:] + SETTINGS[:r % 3]:
            run(setting, WARMUP)                      # this setting's own warm-up
            v, seg_ms, resident = run(setting, BATCHES)
            rate[setting].append(v)
            ms[setting] += seg_ms
            res[setting] += resident
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    # the quantile kernel against fetching the window and scanning it on the host
    win = min(num_sites, 1 << 20)
    probs = (0.25, 0.5, 0.75)
    t_dev, t_host = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        q = al.site_quantiles(probs, 0, win)
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        lv = al.site_histogram(0, win)["level"]
        t_fetch = time.perf_counter() - t0
        c = np.cumsum(lv, axis=1, dtype=np.uint64)
        n = c[:, -1]
        bins_host = []
        for p in probs:
            k = np.minimum(np.maximum(np.ceil(p * n.astype(np.float64)).astype(np.uint64), 1), n)
            bins_host.append(np.where(n > 0, np.argmax(c >= k[:, None], axis=1), 0xFFFFFFFF))
        t_host.append((time.perf_counter() - t0, t_fetch))
        assert all(np.array_equal(q["bin"][:, i], b.astype(np.uint32)) for i, b in enumerate(bins_host)) and np.array_equal(q["n"], n.astype(np.uint32))
    totals = al.site_summary(0, 0)["totals"]
    stats = al.session_stats()
    al.close()
    m = {s: med(rate[s]) for s in SETTINGS}
    seg = {s: med(ms[s]) for s in SETTINGS}
    return {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight; ids: %s over %d sites; bins %d" % (DEPTH, name, num_sites, BINS),
            "batches_each": BATCHES, "reps": REPS, "msamp_s": {s: [round(v, 1) for v in rate[s]] for s in SETTINGS},
            "median": {s: round(m[s], 1) for s in SETTINGS}, "ratio_hist_over_summary": round(m["hist"] / m["summary"], 4),
            "ratio_summary_over_off": round(m["summary"] / m["off"], 4),
            "segment_stage_ms_per_batch": {s: round(seg[s], 3) for s in SETTINGS},
            "histogram_ms_per_batch": round(seg["hist"] - seg["summary"], 3), "summary_ms_per_batch": round(seg["summary"] - seg["off"], 3),
            "resident_tickets": res, "table_bytes": 56 * num_sites, "histogram_bytes": 4 * (BINS + 18) * num_sites,
            "quantiles": {"window_sites": win, "probs": list(probs), "device_ms_best_of_3": round(1e3 * min(t_dev), 3),
                          "fetch_and_numpy_ms_best_of_3": round(1e3 * min(t for t, _ in t_host), 3),
                          "of_which_fetch_ms": round(1e3 * min(f for _, f in t_host), 3)},
            "totals": totals, "session_stats": {k: stats[k] for k in ("sessions", "tickets", "reads", "aborted", "republished")}}


rec = {name: measure(name, n) for name, n in PATTERNS.items()}
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
