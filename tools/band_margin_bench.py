#!/usr/bin/env python
"""GPU box: what the band-margin diagnostics (Aligner.set_band_margin) cost on the async align line. cfg2's shape (1 024 reads
x ~20 k samples, syn9, band 400) and cfg2_polya through align_async in steady state (DEPTH tickets in flight), the switch
alternating off / on every ROUND batches in one process, BATCHES of each after a warm-up. Per workload: Msamp/s for both and
the ratio; the per-segment stage's time per batch from the library's HIP events (dyn_timing: ms_total - ms_dp, the events
around launch_segments) off and on -- their difference is what k_bmargin_init / k_bmargin take; session_stats, which shows
that the tickets stayed in the resident session; how many reads of the last ticket touched a real band edge. Prints one JSON
line and writes it to argv[1] if given (profiles/band_margin/cost.json)."""
import json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("BM_BATCHES", 24))
ROUND = int(os.environ.get("BM_ROUND", 4))
DEPTH = int(os.environ.get("BM_DEPTH", 4))
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)


def measure(name):
    cfg = synth.CONFIGS[name]
    packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"], polya=cfg.get("polya")))
              for j in range(2)]
    samples = [int(p[1][-1]) for p in packed]
    al = Aligner(model, cfg["pore"], band=400, device=0)

    last = (0, 0)

    def run(on, n):
        """n batches with the switch `on`, DEPTH in flight; wall time from the first submit to the last wait"""
        al.set_band_margin(on)
        t0 = time.perf_counter()
        inflight, done, seg_ms, resident = [], 0, [], 0

        def finish(t, k):
            nonlocal done, resident, last
            res = t.wait()
            if on:
                last = (int((res.band_margin_low == 0).sum() + (res.band_margin_high == 0).sum()), int(res.band_edge_rows.sum()))
            tm = t.timing()
            seg_ms.append(tm["ms_total"] - tm["ms_dp"])
            resident += tm["launches"] == 0
            t.close()
            done += samples[k]

        for j in range(n):
            inflight.append((al.align_async(*packed[j % 2], True), j % 2))
            if len(inflight) >= DEPTH:
                finish(*inflight.pop(0))
        for t, k in inflight:
            finish(t, k)
        return done, time.perf_counter() - t0, seg_ms, resident

    run(False, 8)
    run(True, 8)   # warm-up: buffers cached
    tot = {False: [0, 0.0, [], 0], True: [0, 0.0, [], 0]}
    for r in range(BATCHES // ROUND):
        for on in (False, True) if r % 2 == 0 else (True, False):
            s, dt, ms, res = run(on, ROUND)
            tot[on][0] += s
            tot[on][1] += dt
            tot[on][2] += ms
            tot[on][3] += res
    off, on = (tot[k][0] / tot[k][1] / 1e6 for k in (False, True))
    ms_off, ms_on = (sorted(tot[k][2])[len(tot[k][2]) // 2] for k in (False, True))
    stats = al.session_stats()
    al.close()
    return {"workload": "%s (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight" % (name, DEPTH),
            "batches_each": BATCHES, "msamp_s_off": round(off, 1), "msamp_s_on": round(on, 1), "ratio_on_off": round(on / off, 4),
            "segment_stage_ms_per_batch_off": round(ms_off, 3), "segment_stage_ms_per_batch_on": round(ms_on, 3),
            "margin_kernels_ms_per_batch": round(ms_on - ms_off, 3),
            "resident_tickets_off": tot[False][3], "resident_tickets_on": tot[True][3],
            "last_ticket_margins_of_0": last[0], "last_ticket_edge_rows": last[1],
            "session_stats": {k: stats[k] for k in ("sessions", "tickets", "reads", "aborted", "republished")}}


rec = {name: measure(name) for name in ("cfg2", "cfg2_polya")}
print(json.dumps(rec))
if len(sys.argv) > 1:
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
