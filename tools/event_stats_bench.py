#!/usr/bin/env python
"""GPU box: what the per-segment signal levels (Aligner.set_event_stats) cost on the async align line. cfg2's shape (1 024 reads
x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), the switch alternating off / on
every ROUND batches in one process, BATCHES of each after a warm-up; prints one JSON line (Msamp/s for both, the ratio) and
writes it to argv[1] if given. The kernels' own time per batch: run this under `rocprofv3 --kernel-trace --stats`
(k_event_short / k_event_long). `event_stats_bench.py cli [out.json]`: the CLI end to end without / with --event-stats."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamont_amd import Aligner, synth

if len(sys.argv) > 1 and sys.argv[1] == "cli":
    # the CLI end to end on 4 096 cfg2-sized reads: the same dataset without and with --event-stats, alternating, in fresh
    # processes (a cold start each); wall time and output size (the rows grow by ~30 B, compressing them costs more)
    import subprocess
    d = tempfile.mkdtemp(prefix="dyn_ev_cli_")
    model = synth.write_model(os.path.join(d, "m9.model"), 9)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(5, 4096, "rna004", mean, sd, 2000)
    raw, bam, _ = synth.write_dataset(os.path.join(d, "in"), "ds", reads, "rna004", seed=1)
    samples = sum(len(r.signal) for r in reads)
    del reads
    res = {False: [], True: []}
    size = {}
    for rep in range(3):
        for on in (False, True):
            out = os.path.join(d, "ev.csv" if on else "plain.csv")
            cmd = [sys.executable, "-m", "dynamont_amd.segmentation.segment", "-r", os.path.join(d, "in"), "-b", bam, "-o", out,
                   "--mode", "basic", "-p", "rna004", "--model_path", model, "--batch-reads", "1024"] + (["--event-stats"] if on else [])
            t0 = time.perf_counter()
            subprocess.run(cmd, check=True, capture_output=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
            res[on].append(time.perf_counter() - t0)
            size[on] = os.path.getsize(out + ".zst")
    rec = {"workload": "dynamont-resquiggle, 4096 reads x ~20 k samples (rna004, syn9), cold process per run",
           "msamples": round(samples / 1e6, 1), "wall_s_off": [round(x, 3) for x in res[False]],
           "wall_s_on": [round(x, 3) for x in res[True]], "zst_mb_off": round(size[False] / 1e6, 2), "zst_mb_on": round(size[True] / 1e6, 2),
           "ratio_best_on_off": round(min(res[True]) / min(res[False]), 4)}
    print(json.dumps(rec))
    if len(sys.argv) > 2:
        json.dump(rec, open(sys.argv[2], "w"), indent=1)
    sys.exit(0)

BATCHES = int(os.environ.get("EV_BATCHES", 24))
ROUND = int(os.environ.get("EV_ROUND", 4))
DEPTH = int(os.environ.get("EV_DEPTH", 4))
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"])) for j in range(2)]
samples = [int(p[1][-1]) for p in packed]
al = Aligner(model, cfg["pore"], band=400, device=0)


def run(on, n):
    """n batches with the switch `on`, DEPTH in flight; wall time from the first submit to the last wait"""
    al.set_event_stats(on)
    t0 = time.perf_counter()
    inflight, done = [], 0
    for j in range(n):
        inflight.append((al.align_async(*packed[j % 2], True), j % 2))
        if len(inflight) >= DEPTH:
            t, k = inflight.pop(0)
            t.wait(); t.close(); done += samples[k]
    for t, k in inflight:
        t.wait(); t.close(); done += samples[k]
    return done, time.perf_counter() - t0


run(False, 8)
run(True, 8)   # warm-up: buffers of both kinds cached
tot = {False: [0, 0.0], True: [0, 0.0]}
for r in range(BATCHES // ROUND):
    for on in (False, True) if r % 2 == 0 else (True, False):
        s, dt = run(on, ROUND)
        tot[on][0] += s
        tot[on][1] += dt
off, on = (tot[k][0] / tot[k][1] / 1e6 for k in (False, True))
rec = {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight" % DEPTH,
       "batches_each": BATCHES, "msamp_s_off": round(off, 1), "msamp_s_on": round(on, 1), "ratio_on_off": round(on / off, 4)}
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
al.close()
