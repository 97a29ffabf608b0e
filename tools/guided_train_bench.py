#!/usr/bin/env python
"""GPU box: what guided-band training (Aligner.train_batch_guided) costs beside the two things a user has today for reads whose
path leaves the band around the diagonal, and how far each one's statistics are from the whole lattice's. Reads: those of
tools/guided_band_bench.py (GB_READS reads of ~2 000 k-mers at ~6 samples per k-mer, one segment stalled for 0.3-0.5 of the read;
syn5, dna_r9). Timed, each after a warm-up run of its own, GB_REPEATS times (median; host clock around the synchronous call, which
ends in a device synchronise and includes upload and fetch; plus the library's HIP events):
  band_400   train_batch at band 400 (the tuned sweeps)
  band_4093  train_batch at band 4093 (the generic wide-band kernel at half band N / 2: the yardstick)
  guided     train_batch_guided at half_width 64 around guide_from_starts(true starts)
Per mode: seconds, lattice cells, the peak lattice memory the library allocated (dyn_batch_arena_bytes: workgroups x the largest
read's arena; band 400: the page pool of the launch) and sum_k |w[k] - w_4093[k]| / S per read, summed over the reads and its
largest value (w: a read's per-k-mer posterior weight, S its samples). Prints one JSON line and writes it to argv[1]
(profiles/guided_train/bench.json)."""
import json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_band_cases as gc
from dynamont_amd import Aligner, synth

READS = int(os.environ.get("GB_READS", 128))
REPEATS = int(os.environ.get("GB_REPEATS", 3))
HALF_WIDTH = 64
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn5.model"), 5, seed=7, stdev=0.25)
_, mean, sd = synth.read_model_file(model)
mean_code, sd_code = synth.code_order_table(mean, sd, gc.K, False)
rng = np.random.default_rng(20261019)
reads = [gc.make_read(rng, mean_code, sd_code, int(rng.integers(1800, 2201)), 6.0, stall=float(rng.uniform(0.3, 0.5))) for _ in range(READS)]
sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
guides = np.concatenate([gc.true_guide(r) for r in reads])
T = np.array([len(r.signal) + 1 for r in reads], dtype=np.int64)
Ncol = np.array([r.n_kmers + 1 for r in reads], dtype=np.int64)


def timed(fn):
    fn()  # warm-up: code objects loaded, buffers cached
    out, secs = None, []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return out, sorted(secs)[len(secs) // 2], secs


def run(al, guided):
    with al.batch(sig, seq) as b:
        if guided:
            b.set_guide(guides, HALF_WIDTH)
            b.train_guided()
        else:
            b.train()
        return b.fetch_train(), b.timing(), b.arena_bytes()


def weights(res, K):
    """[reads, K] per-k-mer posterior weights (a failed read: zeros)"""
    w = np.zeros((READS, K))
    for i in range(READS):
        a = int(res.em_offsets[i])
        n = int(res.em_count[i])
        w[i, res.em_code[a:a + n]] = res.em_weight[a:a + n]
    return w


rec = {"workload": "%d stalled reads, %d samples, %d k-mers (syn5, dna_r9)" % (READS, int(T.sum() - READS), int(Ncol.sum() - READS)),
       "repeats": REPEATS}
out = {}
for name, band, guided in (("band_400", 400, False), ("band_4093", 4093, False), ("guided_half_width_64", 400, True)):
    al = Aligner(model, gc.PORE, band=band, device=0)
    (res, tm, arena), s, every = timed(lambda: run(al, guided))
    row = {"seconds": round(s, 4), "seconds_all": [round(x, 4) for x in every], "device_ms": round(tm["ms_total"], 3), "cells": int(tm["cells"]),
           "reads_ok": int((res.status == 0).sum())}
    if arena:
        row["peak_arena_bytes"] = int(arena)
    else:
        row["page_pool_bytes"] = int(tm["pool_pages"]) * int(tm["page_rows"]) * 448 * 8
    out[name] = weights(res, al.num_kmers)
    rec[name] = row
    al.close()
S = (T - 1).astype(np.float64)
for name in ("band_400", "band_4093", "guided_half_width_64"):
    per_read = np.abs(out[name] - out["band_4093"]).sum(axis=1) / S
    rec[name]["weight_shift_sum"] = float(per_read.sum())
    rec[name]["weight_shift_max"] = float(per_read.max())
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
