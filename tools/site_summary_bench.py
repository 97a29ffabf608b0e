#!/usr/bin/env python
"""GPU box: what the per-site level summary (Aligner.set_site_summary + site_ids=) costs on the async align line. cfg2's shape
(1 024 reads x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), the switch
alternating off / on in ONE process, each setting after its own warm-up, REPS times; the median of the repetitions is reported.
Two id patterns: `uniform` -- every read a window of consecutive sites at a random start among 10^8 sites (a 5.6 GB table, hardly
any two rows on one cell); `hot` -- every read on one 2 000-site transcript (1 024 adds per cell per batch: the worst case for
contention). Per pattern: Msamp/s off and on and their ratio; the per-segment stage's time per batch from the library's HIP
events (dyn_timing: ms_total - ms_dp) off and on -- their difference is what k_ssum_short / k_ssum_long take; the table's totals;
session_stats, which shows that the tickets stayed in the resident session. The yardstick is the OFF line of the same process.
Prints one JSON line and writes it to argv[1] if given (profiles/site_summary/cost.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("SS_BATCHES", 12))
WARMUP = int(os.environ.get("SS_WARMUP", 4))
REPS = int(os.environ.get("SS_REPS", 3))
DEPTH = int(os.environ.get("SS_DEPTH", 4))
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
    al = Aligner(model, cfg["pore"], band=400, device=0)

    def run(on, n):
        """n batches with the switch `on`, DEPTH in flight; wall time from the first submit to the last wait"""
        al.set_site_summary(num_sites if on else 0)
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
            inflight.append((al.align_async(*packed[j % 2], True, site_ids=ids[j % 2] if on else None), j % 2))
            if len(inflight) >= DEPTH:
                finish(*inflight.pop(0))
        for t, k in inflight:
            finish(t, k)
        return done / (time.perf_counter() - t0) / 1e6, seg_ms, resident

    rate = {False: [], True: []}
    ms = {False: [], True: []}
    res = {False: 0, True: 0}
    for r in range(REPS):
        for on in (False, True) if r % 2 == 0 else (True, False):
            run(on, WARMUP)                       # this setting's own warm-up: buffers cached, the table allocated
            v, seg_ms, resident = run(on, BATCHES)
            rate[on].append(v)
            ms[on] += seg_ms
            res[on] += resident
    med = lambda x: sorted(x)[len(x) // 2]  # noqa: E731
    totals = al.site_summary(0, 0)["totals"]
    stats = al.session_stats()
    al.close()
    off, on = med(rate[False]), med(rate[True])
    return {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight; ids: %s over %d sites" % (DEPTH, name, num_sites),
            "batches_each": BATCHES, "reps": REPS, "msamp_s_off": [round(v, 1) for v in rate[False]], "msamp_s_on": [round(v, 1) for v in rate[True]],
            "median_off": round(off, 1), "median_on": round(on, 1), "ratio_on_off": round(on / off, 4),
            "segment_stage_ms_per_batch_off": round(med(ms[False]), 3), "segment_stage_ms_per_batch_on": round(med(ms[True]), 3),
            "summary_kernels_ms_per_batch": round(med(ms[True]) - med(ms[False]), 3),
            "resident_tickets_off": res[False], "resident_tickets_on": res[True], "table_bytes": 56 * num_sites, "totals": totals,
            "session_stats": {k: stats[k] for k in ("sessions", "tickets", "reads", "aborted", "republished")}}


rec = {name: measure(name, n) for name, n in PATTERNS.items()}
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
