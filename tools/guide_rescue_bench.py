#!/usr/bin/env python
"""GPU box: what the guide rescue (Aligner.set_guide_rescue: the plain alignment of every read, then a self-guided second
alignment of only the reads whose band margin flags them, inside the same ticket) costs beside the modes that exist without it.
Workload: GR_READS (1 024) reads of ~2 000 k-mers and ~20 k samples (syn5, dna_r9, band 400), of which GR_STALLED (0 / 16 / 128)
are the stalled family of tools/auto_guide_bench.py and the rest plain reads of the same size. One ticket per run (submit +
wait, host clock, upload and the copies home included); every mode after a warm-up run of its own, GR_REPEATS (3) times, median;
all in this one process:
  a_plain_margins_sessions_off   plain tickets with set_band_margin(True), resident sessions off
  b_plain_margins_sessions_on    the same with sessions on
  c_auto_guide_every_read        set_auto_guide(64, 8): every read self-guided
  d_guide_rescue                 set_guide_rescue(1, 64, 8)
  c_flagged_only                 (GR_STALLED > 0) set_auto_guide(64, 8) over the reads (d) flagged alone: what (d) adds to (a) at best
Per mode: seconds per ticket (median, all, spread = max - min), the checked reads that carry the borders of band 4093 (checked:
every stalled read and the first 64 others, aligned once on a band-4093 handle), reads flagged / rescued, peak arena bytes.
(a) - (c) exist without the rescue and are the yardsticks; (d) is never its own. Condition at GR_STALLED = 0: (d) within (a) plus
twice (a)'s spread -- recorded as d_within_a_plus_twice_its_spread. Prints one JSON line and writes it to argv[1]."""
import json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_band_cases as gc
from dynamont_amd import Aligner, synth
from dynamont_amd._dynamont import Batch

READS = int(os.environ.get("GR_READS", 1024))
STALLED = int(os.environ.get("GR_STALLED", 16))
REPEATS = int(os.environ.get("GR_REPEATS", 3))
M, HW, REFINE, CHECK_PLAIN = 1, 64, 8, 64
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn5.model"), 5, seed=7, stdev=0.25)
_, mean, sd = synth.read_model_file(model)
mean_code, sd_code = synth.code_order_table(mean, sd, gc.K, False)
rng = np.random.default_rng(20261019)
stalled = [gc.make_read(rng, mean_code, sd_code, int(rng.integers(1800, 2201)), 6.0, stall=float(rng.uniform(0.3, 0.5))) for _ in range(STALLED)]
rng = np.random.default_rng(20261020)
others = [gc.make_read(rng, mean_code, sd_code, int(rng.integers(1800, 2201)), 9.0) for _ in range(READS - STALLED)]
step = max(1, READS // max(1, STALLED))
reads, stalled_at = list(others), []
for k, r in enumerate(stalled):                      # the stalled reads spread over the ticket
    reads.insert(k * step, r)
    stalled_at.append(k * step)
pack = synth.pack_reads([synth.SynthRead(r.signal, r.sequence) for r in reads])
checked = sorted(set(stalled_at) | set([i for i in range(READS) if i not in set(stalled_at)][:CHECK_PLAIN]))

widest = Aligner(model, gc.PORE, band=4093, device=0)
ref = widest.align_batch([reads[i].signal for i in checked], [reads[i].sequence for i in checked])
widest.close()


def borders_of_4093(res, idx=None):
    """how many of the checked reads carry band 4093's borders; idx: res holds the reads idx of the ticket"""
    where = {r: k for k, r in enumerate(range(READS) if idx is None else idx)}
    n = 0
    for k, i in enumerate(checked):
        if i not in where or ref.status[k] != 0 or res.status[where[i]] != 0:
            continue
        a, b, m = int(res.seg_offsets[where[i]]), int(ref.seg_offsets[k]), int(ref.n_segments[k])
        n += int(res.n_segments[where[i]]) == m and np.array_equal(res.signal_positions[a:a + m], ref.signal_positions[b:b + m])
    return n


al = Aligner(model, gc.PORE, band=400, device=0)
rec = {"workload": "%d reads (%d stalled), %d samples, %d k-mers (syn5, dna_r9, band 400); min margin %d, half width %d, refine %d" %
       (READS, STALLED, sum(len(r.signal) for r in reads), sum(r.n_kmers for r in reads), M, HW, REFINE),
       "repeats": REPEATS, "checked_reads": len(checked)}


def ticket(setup, pk=pack):
    def run():
        setup(True)
        t = al.align_async(*pk)
        setup(False)
        res = t.wait()
        out = (res, Batch.arena_bytes(t))
        t.close()
        return out
    return run


def row(name, fn, idx=None):
    fn()  # warm-up: code objects loaded, buffers cached, the pipeline's threads started
    secs = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        res, arena = fn()
        secs.append(time.perf_counter() - t0)
    r = {"seconds": round(sorted(secs)[len(secs) // 2], 4), "seconds_all": [round(x, 4) for x in secs], "spread": round(max(secs) - min(secs), 4),
         "reads_ok": int((res.status == 0).sum()), "checked_reads_with_the_borders_of_band_4093": borders_of_4093(res, idx),
         "peak_arena_bytes": int(arena)}
    if res.rescue is not None:
        r["flagged"] = int((res.rescue != 0).sum())
        r["rescued"] = int((res.rescue == 1).sum())
        r["left_code_2_or_3"] = int((res.rescue >= 2).sum())
        r["not_converged"] = int(((res.rescue == 1) & (res.guide_converged == 0)).sum())
    rec[name] = r
    print(name, json.dumps(r), flush=True)
    return res


al.set_band_margin(True)
al.set_session_mode(False)
row("a_plain_margins_sessions_off", ticket(lambda on: None))
al.set_session_mode(True)
row("b_plain_margins_sessions_on", ticket(lambda on: None))
al.set_session_mode(False)
row("c_auto_guide_every_read", ticket(lambda on: al.set_auto_guide(HW if on else 0, REFINE)))
res_d = row("d_guide_rescue", ticket(lambda on: al.set_guide_rescue(M, HW if on else 0, REFINE)))
flagged = np.flatnonzero(res_d.rescue == 1).tolist()
if flagged:
    sub = synth.pack_reads([synth.SynthRead(reads[i].signal, reads[i].sequence) for i in flagged])
    row("c_flagged_only", ticket(lambda on: al.set_auto_guide(HW if on else 0, REFINE), sub), idx=flagged)
    rec["a_plus_c_flagged_only"] = round(rec["a_plain_margins_sessions_off"]["seconds"] + rec["c_flagged_only"]["seconds"], 4)
a = rec["a_plain_margins_sessions_off"]
rec["d_minus_a"] = round(rec["d_guide_rescue"]["seconds"] - a["seconds"], 4)
rec["d_within_a_plus_twice_its_spread"] = bool(rec["d_guide_rescue"]["seconds"] <= a["seconds"] + 2 * a["spread"])
al.close()
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
