#!/usr/bin/env python
"""GPU box: what the SPARSE per-site table (Aligner.set_site_summary(num_sites, capacity=)) costs on the async align line against
the DENSE table of the same process. The pattern of tools/site_summary_bench.py: cfg2's shape (1 024 reads x ~20 k samples, syn9,
band 400) through align_async in steady state (DEPTH tickets in flight), the settings alternating in ONE process, each after its
own warm-up, REPS times; medians are reported. Settings: `off` (no table), `dense` (the existing path: the yardstick) and the
sparse table at load factors 0.25, 0.5 and 0.8 -- capacity = distinct ids of the two batches / load. Two id patterns: `uniform`
-- every read a window of consecutive sites at a random start among 10^8 sites; `hot` -- every read on one 2 000-site transcript.
The two batches repeat, so after a setting's warm-up every key is in the map: the steady state prices the probes of a lookup; the
inserts fall into the warm-up. Per setting: Msamp/s, its ratio to dense, the per-segment stage's ms per batch from the library's
HIP events (dyn_timing: ms_total - ms_dp), the map's statistics. Prints one JSON line and writes it to argv[1] if given
(profiles/site_map/cost.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("SM_BATCHES", 12))
WARMUP = int(os.environ.get("SM_WARMUP", 4))
REPS = int(os.environ.get("SM_REPS", 3))
DEPTH = int(os.environ.get("SM_DEPTH", 4))
LOADS = (0.25, 0.5, 0.8)
PATTERNS = {"uniform": 100_000_000, "hot": 2_000}
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
    distinct = int(np.unique(np.concatenate(ids)).size)
    settings = {"off": None, "dense": 0}
    settings.update({"sparse_%g" % lf: max(int(distinct / lf) + 1, 8) for lf in LOADS})
    al = Aligner(model, cfg["pore"], band=400, device=0)

    def run(setting, n):
        """n batches under `setting`, DEPTH in flight; wall time from the first submit to the last wait"""
        cap = settings[setting]
        if cap is None:
            al.set_site_summary(0)
        else:
            al.set_site_summary(num_sites, capacity=cap or None)
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
            inflight.append((al.align_async(*packed[j % 2], True, site_ids=None if cap is None else ids[j % 2]), j % 2))
            if len(inflight) >= DEPTH:
                finish(*inflight.pop(0))
        for t, k in inflight:
            finish(t, k)
        return done / (time.perf_counter() - t0) / 1e6, seg_ms

    rate = {s: [] for s in settings}
    ms = {s: [] for s in settings}
    maps = {}
    order = list(settings)
    for r in range(REPS):
        for s in order if r % 2 == 0 else order[::-1]:
            run(s, WARMUP)                       # this setting's own warm-up: buffers cached, the table allocated, the keys inserted
            v, seg_ms = run(s, BATCHES)
            rate[s].append(v)
            ms[s] += seg_ms
            if s.startswith("sparse"):
                maps[s] = al.site_map()
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    al.close()
    dense = med(rate["dense"])
    out = {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight; ids: %s over %d sites, %d distinct"
                       % (DEPTH, name, num_sites, distinct), "batches_each": BATCHES, "reps": REPS,
           "dense_spread": round((max(rate["dense"]) - min(rate["dense"])) / dense, 4)}
    for s in settings:
        out[s] = {"msamp_s": [round(v, 1) for v in rate[s]], "median": round(med(rate[s]), 1), "ratio_to_dense": round(med(rate[s]) / dense, 4),
                  "segment_stage_ms_per_batch": round(med(ms[s]), 3)}
        if s in maps:
            out[s]["map"] = maps[s]
            out[s]["bytes"] = maps[s]["capacity"] * 60
    out["dense"]["bytes"] = 56 * num_sites
    return out


rec = {name: measure(name, n) for name, n in PATTERNS.items()}
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
