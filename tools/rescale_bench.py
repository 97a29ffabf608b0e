#!/usr/bin/env python
"""GPU box: what the per-read signal rescaling (Aligner.set_rescale) costs on the async align line. cfg2's shape (1 024 reads
x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), K = 0, 1 and 2 alternating
every ROUND batches in one process, BATCHES of each after a warm-up; prints one JSON line (Msamp/s of every K, the ratios to
K = 0, the per-batch timing of the library for every K) and writes it to argv[1] if given. The kernels' own time per batch:
run this under `rocprofv3 --kernel-trace --stats` (k_rescale_fit / k_rescale_apply / k_rescale_init against k_read_queue)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("RS_BATCHES", 12))
ROUND = int(os.environ.get("RS_ROUND", 4))
DEPTH = int(os.environ.get("RS_DEPTH", 4))
KS = (0, 1, 2)
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"])) for j in range(2)]
samples = [int(p[1][-1]) for p in packed]
al = Aligner(model, cfg["pore"], band=400, device=0)


def run(K, n, timings=None):
    """n batches with K iterations, DEPTH in flight; wall time from the first submit to the last wait"""
    al.set_rescale(K)
    t0 = time.perf_counter()
    inflight, done = [], 0

    def finish(t, k):
        t.wait()
        if timings is not None:
            timings.append(t.timing())
        t.close()
        return samples[k]

    for j in range(n):
        inflight.append((al.align_async(*packed[j % 2], True), j % 2))
        if len(inflight) >= DEPTH:
            done += finish(*inflight.pop(0))
    for t, k in inflight:
        done += finish(t, k)
    return done, time.perf_counter() - t0


for K in KS:   # warm-up: buffers of every kind cached
    run(K, 4)
tot = {K: [0, 0.0] for K in KS}
tim = {K: [] for K in KS}
for r in range(BATCHES // ROUND):
    for K in (KS if r % 2 == 0 else KS[::-1]):
        s, dt = run(K, ROUND, tim[K])
        tot[K][0] += s
        tot[K][1] += dt
rate = {K: tot[K][0] / tot[K][1] / 1e6 for K in KS}


def mean_of(K, key):
    v = [t[key] for t in tim[K]]
    return round(sum(v) / len(v), 3) if v else None


rec = {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight" % DEPTH,
       "batches_each": BATCHES,
       "msamp_s": {str(K): round(rate[K], 1) for K in KS},
       "ratio_to_K0": {str(K): round(rate[K] / rate[0], 4) for K in KS},
       "library_ms_per_batch": {str(K): {"ms_dp": mean_of(K, "ms_dp"), "ms_total": mean_of(K, "ms_total"),
                                         "launches": mean_of(K, "launches")} for K in KS}}
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
al.close()
