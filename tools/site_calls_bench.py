#!/usr/bin/env python
"""GPU box: what the per-read site calls (Aligner.set_site_calls) cost on the async align line against the SAME process with the
per-site summary on and the calls off -- the existing code path, the yardstick. The pattern of tools/site_map_bench.py: cfg2's shape
(1 024 reads x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), the settings
alternating in ONE process, each after its own warm-up, REPS times; medians are reported. Two id patterns: `hot` -- every read on
one 2 000-site transcript, a dense table; `scattered` -- every read a window of consecutive sites at a random start among 10^8
sites, a sparse table at load 0.5 (the model's rows take their buckets at the upload, the batches' ids theirs in the warm-up). Every
id the batches name has a two-component model row. Per setting: Msamp/s, the ratio to the yardstick, the per-segment stage's ms per
batch from the library's HIP events (dyn_timing: ms_total - ms_dp). For comparison the HOST route for one batch: level_mean
fetched (set_event_stats), the model gathered by id and the same E-step formed in NumPy -- its wall time. Prints one JSON line and
writes it to argv[1] if given (profiles/site_calls/cost.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("SC_BATCHES", 12))
WARMUP = int(os.environ.get("SC_WARMUP", 4))
REPS = int(os.environ.get("SC_REPS", 3))
DEPTH = int(os.environ.get("SC_DEPTH", 4))
PATTERNS = {"hot": 2_000, "scattered": 100_000_000}
COLUMNS = ("pi1", "mu0", "mu1", "var0", "var1")
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"])) for j in range(2)]
samples = [int(p[1][-1]) for p in packed]
K = 9


def make_ids(seq_off, num_sites, rng):
    lens = np.diff(seq_off.astype(np.int64))
    out = np.empty(int(seq_off[-1]), dtype=np.uint32)
    for i, n in enumerate(lens.tolist()):
        start = 0 if num_sites <= n else int(rng.integers(0, num_sites - n))
        out[int(seq_off[i]):int(seq_off[i]) + n] = (start + np.arange(n)) % num_sites
    return out


def upload(al, distinct, num_sites, rng):
    """a two-component row for every id of `distinct` (ascending), a 2^20 window of the id space at a time"""
    stored = dropped = 0
    step = 1 << 20
    for w0 in np.unique(distinct // step).tolist():
        lo, hi = w0 * step, min((w0 + 1) * step, num_sites)
        at = distinct[(distinct >= lo) & (distinct < hi)] - lo
        m = {k: np.zeros(hi - lo) for k in COLUMNS}
        mu = rng.uniform(-1.0, 1.0, at.size)
        for k, v in zip(COLUMNS, (rng.uniform(0.1, 0.9, at.size), mu, mu + rng.uniform(0.3, 0.9, at.size), rng.uniform(0.02, 0.2, at.size),
                                  rng.uniform(0.02, 0.2, at.size))):
            m[k][at] = v
        got = al.set_site_model(lo, m)
        stored += got["stored"]
        dropped += got["dropped"]
    return stored, dropped


def host_route(res, ids, seq_off, model_cols):
    """what the calls replace: the batch's level_mean on the host, the model gathered by id, the E-step in NumPy; seconds"""
    t0 = time.perf_counter()
    row_id = np.full(res.cap, 0xFFFFFFFF, dtype=np.uint32)
    so = seq_off.astype(np.int64)
    for i in range(res.n):
        if res.status[i] == 0:
            a, n = int(res.seg_offsets[i]), int(res.n_segments[i])
            row_id[a:a + n] = ids[so[i] + K // 2:so[i] + K // 2 + n]
    ok = row_id != 0xFFFFFFFF
    pi1, mu0, mu1, var0, var1 = (model_cols[k][row_id[ok]] for k in COLUMNS)
    m = res.level_mean[ok]
    with np.errstate(all="ignore"):
        q0, q1 = -0.5 * ((m - mu0) ** 2 / var0), -0.5 * ((m - mu1) ** 2 / var1)
        qm = np.maximum(q0, q1)
        p0, p1 = (1.0 - pi1) / np.sqrt(var0) * np.exp(q0 - qm), pi1 / np.sqrt(var1) * np.exp(q1 - qm)
        prob = p1 / (p0 + p1)
        z = (m - mu0) / np.sqrt(var0)
    return time.perf_counter() - t0, int(ok.sum()), float(np.nanmean(prob)), float(np.nanmean(z))


def measure(name, num_sites):
    rng = np.random.default_rng(11)
    ids = [make_ids(p[3], num_sites, rng) for p in packed]
    distinct = np.unique(np.concatenate(ids)).astype(np.int64)
    sparse = num_sites > 10_000_000
    cap = int(distinct.size / 0.5) + 1 if sparse else None
    al = Aligner(model, cfg["pore"], band=400, device=0)
    al.set_site_summary(num_sites, capacity=cap)
    stored, dropped = upload(al, distinct, num_sites, rng)
    settings = ("summary", "calls")

    def run(setting, n):
        al.set_site_calls(setting == "calls")
        t0 = time.perf_counter()
        inflight, done, seg_ms = [], 0, []

        def finish(t, k):
            nonlocal done
            t.wait()
            tm = t.timing()
            seg_ms.append(tm["ms_total"] - tm["ms_dp"])
            t.close()
            done += samples[k]

        for j in range(n):
            inflight.append((al.align_async(*packed[j % 2], True, site_ids=ids[j % 2]), j % 2))
            if len(inflight) >= DEPTH:
                finish(*inflight.pop(0))
        for t, k in inflight:
            finish(t, k)
        return done / (time.perf_counter() - t0) / 1e6, seg_ms

    rate = {s: [] for s in settings}
    ms = {s: [] for s in settings}
    for r in range(REPS):
        for s in settings if r % 2 == 0 else settings[::-1]:
            run(s, WARMUP)                       # this setting's own warm-up: buffers cached, the keys of the ids inserted
            v, seg_ms = run(s, BATCHES)
            rate[s].append(v)
            ms[s] += seg_ms
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    base = med(rate["summary"])
    out = {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight; ids: %s over %d sites, %d distinct, %s table"
                       % (DEPTH, name, num_sites, distinct.size, "sparse (capacity %d)" % cap if sparse else "dense"),
           "batches_each": BATCHES, "reps": REPS, "model_rows_uploaded": stored, "model_rows_dropped": dropped,
           "summary_spread": round((max(rate["summary"]) - min(rate["summary"])) / base, 4)}
    for s in settings:
        out[s] = {"msamp_s": [round(v, 1) for v in rate[s]], "median": round(med(rate[s]), 1), "ratio_to_summary": round(med(rate[s]) / base, 4),
                  "segment_stage_ms_per_batch": round(med(ms[s]), 3)}
    if sparse:
        out["map"] = al.site_map()
    else:
        # the host route, one batch: what it costs to form the same two columns from level_mean on the host
        al.set_site_calls(False)
        al.set_event_stats(True)
        with al.align_async(*packed[0], True, site_ids=ids[0]) as t:
            res = t.wait()
        sec, rows, mp, mz = host_route(res, ids[0], packed[0][3], al.site_model())
        out["host_route_one_batch"] = {"numpy_ms": round(sec * 1e3, 2), "rows": rows, "level_mean_bytes_to_the_host": 8 * int(res.cap),
                                       "mean_probability": round(mp, 4), "mean_z": round(mz, 4)}
        al.set_event_stats(False)
    al.close()
    return out


rec = {name: measure(name, n) for name, n in PATTERNS.items()}
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
