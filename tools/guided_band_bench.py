#!/usr/bin/env python
"""GPU box: what the guided band (Aligner.align_batch_guided) costs beside the two things a user has today for reads whose path
leaves the band around the diagonal. Reads: the stall family of tests/guided_band_cases.py scaled to ~20 k samples (GB_READS reads
of ~2 000 k-mers at ~6 samples per k-mer, one segment stalled for 0.3-0.5 of the read; syn5, dna_r9). Timed, each after a warm-up
run of its own, GB_REPEATS times (median; host clock around the synchronous call, which ends in a device synchronise and includes
upload and fetch; plus the library's HIP events where one launch makes up the call):
  plain   align_batch at band 400 (most of these reads run along the band's edge: this is the cost, not the answer)
  retry   align_batch with set_band_retry(1): band x 2 until every margin passes (the generic wide-band kernel above band 447)
  guided  align_batch_guided at half_width 64 around guide_from_starts(true starts)
Per mode: seconds, lattice cells (T x band columns, every pass) and the peak lattice memory the library allocated
(dyn_batch_arena_bytes: workgroups x the largest read's arena; for the retry, of its last and widest pass, run once more on a handle
of that band; plain: the page pool of the launch). Untimed, as the yardstick for the answers: the same reads at band 4093 (half band
N / 2, ~1 000 columns either side of the diagonal, far beyond any of these stalls), and per mode the reads whose borders equal it.
Prints one JSON line and writes it to argv[1] (profiles/guided_band/bench.json)."""
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
guides = [gc.true_guide(r) for r in reads]
T = np.array([len(r.signal) + 1 for r in reads], dtype=np.int64)
Ncol = np.array([r.n_kmers + 1 for r in reads], dtype=np.int64)


def cells_at(band, idx):
    return int((T[idx] * np.minimum(2 * np.minimum(band // 2, Ncol[idx] // 2) + 1, Ncol[idx])).sum())


def timed(fn):
    fn()  # warm-up: code objects loaded, buffers cached, retry handles created
    out, secs = None, []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        out = fn()
        secs.append(time.perf_counter() - t0)
    return out, sorted(secs)[len(secs) // 2], secs


def borders(res, i):
    a = int(res.seg_offsets[i])
    return res.signal_positions[a:a + int(res.n_segments[i])]


al = Aligner(model, gc.PORE, band=400, device=0)
rec = {"workload": "%d stalled reads, %d samples, %d k-mers (syn5, dna_r9)" % (READS, int(T.sum() - READS), int(Ncol.sum() - READS)),
       "repeats": REPEATS}

timing = {}


def plain():
    with al.batch(sig, seq) as b:
        b.align(True)
        timing["plain"] = b.timing()
        return b.fetch()


def guided():
    with al.batch(sig, seq) as b:
        b.set_guide(np.concatenate(guides), HALF_WIDTH)
        b.align(True)
        timing["guided"] = b.timing()
        timing["guided_arena"] = b.arena_bytes()
        return b.fetch()


res_plain, s_plain, all_plain = timed(plain)
tp = timing["plain"]
row_bytes = 448 * (8 if tp["lp_inplace"] else 12) + 56
rec["plain_band_400"] = {"seconds": round(s_plain, 4), "seconds_all": [round(x, 4) for x in all_plain], "device_ms": round(tp["ms_total"], 3),
                         "cells": int(tp["cells"]), "page_pool_bytes": int(tp["pool_pages"]) * int(tp["page_rows"]) * row_bytes}

al.set_band_retry(1)
res_retry, s_retry, all_retry = timed(lambda: al.align_batch(sig, seq))
al.set_band_retry(0)
al.set_band_margin(False)
every = np.arange(READS)
cells, band = cells_at(400, every), 400
while band < int(res_retry.band_used.max()):
    band = min(band * 2, 4093)
    cells += cells_at(band, every[res_retry.band_used >= band])
top = int(res_retry.band_used.max())
rec["retry"] = {"seconds": round(s_retry, 4), "seconds_all": [round(x, 4) for x in all_retry], "cells": cells,
                "band_used": {str(int(k)): int(v) for k, v in zip(*np.unique(res_retry.band_used, return_counts=True))},
                "margin_still_0": int((np.minimum(res_retry.band_margin_low, res_retry.band_margin_high) < 1).sum()),
                "arena_bytes_one_workgroup": int(25 * (T * (2 * np.minimum(top // 2, Ncol // 2) + 3)).max())}
last = [i for i in range(READS) if res_retry.band_used[i] == top]
if top > 400:
    wide_al = Aligner(model, gc.PORE, band=top, device=0)
    with wide_al.batch([sig[i] for i in last], [seq[i] for i in last]) as b:
        b.align(True)
        rec["retry"]["peak_arena_bytes_last_pass"] = b.arena_bytes()
        rec["retry"]["reads_last_pass"] = len(last)
    wide_al.close()

res_guided, s_guided, all_guided = timed(guided)
tg = timing["guided"]
rec["guided_half_width_64"] = {"seconds": round(s_guided, 4), "seconds_all": [round(x, 4) for x in all_guided], "device_ms": round(tg["ms_total"], 3),
                               "cells": int(tg["cells"]), "arena_bytes_one_workgroup": int(25 * T.max() * (2 * HALF_WIDTH + 3)),
                               "peak_arena_bytes": int(timing["guided_arena"]),
                               "reads_ok": int((res_guided.status == 0).sum())}
same = lambda x, y: sum(int(x.status[i] == 0 and y.status[i] == 0 and np.array_equal(borders(x, i), borders(y, i))) for i in range(READS))  # noqa: E731
rec["reads_with_the_retrys_borders"] = {"plain": same(res_plain, res_retry), "guided": same(res_guided, res_retry)}
widest = Aligner(model, gc.PORE, band=4093, device=0)
res_widest = widest.align_batch(sig, seq)
widest.close()
rec["reads_with_the_borders_of_band_4093"] = {"plain": same(res_plain, res_widest), "retry": same(res_retry, res_widest),
                                              "guided": same(res_guided, res_widest), "band_4093_ok": int((res_widest.status == 0).sum())}
rec["ratio_guided_over_retry_seconds"] = round(s_guided / s_retry, 4)
al.close()
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
