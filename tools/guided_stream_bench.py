#!/usr/bin/env python
"""GPU box: what a self-guided TICKET (Aligner.set_auto_guide: every read refined inside one launch, by the workgroup that holds
it) costs beside the synchronous align_batch_auto (the round scheme: a launch per round), on the reads of tools/auto_guide_bench.py:
GS_READS stalled reads of ~2 000 k-mers and ~20 k samples (syn5, dna_r9), half width 64, refine 8. Every mode is timed after a
warm-up run of its own, GS_REPEATS times (median; host clock, upload and the copies home included), all in this one process:
  a_sync_round_scheme     align_batch_auto(signals, sequences, 64, 8)
  b_one_ticket            the same reads as one align_async ticket under set_auto_guide(64, 8): submit + wait
  c_eight_tickets         eight such tickets in flight: submit all, wait for all; seconds per ticket
The answers of (a) and (b) must be equal byte for byte (status, Z, rows, guide_rounds, guide_converged, final guides): the tool
exits with an error if they are not. Prints one JSON line and writes it to argv[1] (profiles/guided_stream/bench.json)."""
import json, os, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_band_cases as gc
from dynamont_amd import Aligner, synth

READS = int(os.environ.get("GS_READS", 128))
REPEATS = int(os.environ.get("GS_REPEATS", 3))
HW, REFINE, IN_FLIGHT = 64, 8, 8
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn5.model"), 5, seed=7, stdev=0.25)
_, mean, sd = synth.read_model_file(model)
mean_code, sd_code = synth.code_order_table(mean, sd, gc.K, False)
rng = np.random.default_rng(20261019)
reads = [gc.make_read(rng, mean_code, sd_code, int(rng.integers(1800, 2201)), 6.0, stall=float(rng.uniform(0.3, 0.5))) for _ in range(READS)]
sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
pack = synth.pack_reads([synth.SynthRead(r.signal, r.sequence) for r in reads])


def timed(fn):
    fn()  # warm-up: code objects loaded, buffers cached, the pipeline's threads started
    secs = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn()
        secs.append(time.perf_counter() - t0)
    return sorted(secs)[len(secs) // 2], secs


def same(x, y):
    """the bytes of two results"""
    if not (np.array_equal(x.status, y.status) and np.array_equal(x.Z.view(np.uint64), y.Z.view(np.uint64)) and
            np.array_equal(x.n_segments, y.n_segments) and np.array_equal(x.seg_offsets, y.seg_offsets)):
        return False
    m = int(x.seg_offsets[-1])
    return all(getattr(x, c)[:m].tobytes() == getattr(y, c)[:m].tobytes() for c in ("signal_positions", "sequence_positions", "probabilities", "states")) and \
        np.array_equal(x.guide_rounds, y.guide_rounds) and np.array_equal(x.guide_converged, y.guide_converged)


al = Aligner(model, gc.PORE, band=400, device=0)
rec = {"workload": "%d stalled reads, %d samples, %d k-mers (syn5, dna_r9), half width %d, refine %d" %
       (READS, sum(len(s) for s in sig), sum(r.n_kmers for r in reads), HW, REFINE), "repeats": REPEATS}


def tickets(n):
    def run():
        al.set_auto_guide(HW, REFINE)
        ts = [al.align_async(*pack) for _ in range(n)]
        al.set_auto_guide(0)
        for t in ts:
            t.wait()
        for t in ts:
            t.close()
    return run


def row(name, fn, per=1):
    s, every = timed(fn)
    rec[name] = {"seconds": round(s / per, 4), "seconds_all": [round(x / per, 4) for x in every]}
    print(name, json.dumps(rec[name]), flush=True)
    return s / per


a = row("a_sync_round_scheme", lambda: al.align_batch_auto(sig, seq, HW, REFINE))
b = row("b_one_ticket", tickets(1))
c = row("c_eight_tickets_per_ticket", tickets(IN_FLIGHT), per=IN_FLIGHT)
rec["b_over_a"] = round(b / a, 4)
rec["c_per_ticket_over_b"] = round(c / b, 4)
# the answers, outside the clock
want = al.align_batch_auto(sig, seq, HW, REFINE, guides=True)
al.set_auto_guide(HW, REFINE)
t = al.align_async(*pack)
al.set_auto_guide(0)
got = t.wait()
guides = t.guide()
rec["a_equals_b_byte_for_byte"] = bool(same(got, want) and all(np.array_equal(x, y) for x, y in zip(guides, want.guides)))
rec["reads_ok"] = int((want.status == 0).sum())
rec["guide_rounds"] = {str(int(k)): int(v) for k, v in zip(*np.unique(want.guide_rounds, return_counts=True))}
rec["not_converged"] = int(((want.guide_converged == 0) & (want.status == 0)).sum())
t.close()
al.close()
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
if not rec["a_equals_b_byte_for_byte"]:
    sys.exit("the ticket's answer differs from the synchronous path's")
