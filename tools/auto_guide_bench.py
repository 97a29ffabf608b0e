#!/usr/bin/env python
"""GPU box: what the self-guided band (Aligner.align_batch_auto, Batch.auto_guide, Batch.set_guide_refine) costs and finds beside
the three rows of tools/guided_band_bench.py, on that tool's reads: AG_READS stalled reads of ~2 000 k-mers and ~20 k samples, one
segment stalled for 0.3-0.5 of the read (syn5, dna_r9). Each mode is timed after a warm-up run of its own, AG_REPEATS times (median;
host clock around the synchronous calls, upload and fetch included):
  plain / retry / guided              as in tools/guided_band_bench.py (guided: half width 64 around the TRUE starts)
  prepass_1_hw64                      auto_guide(64), one alignment
  prepass_refine8_hw64                auto_guide(64), set_guide_refine(8)
  prepass_refine8_hw32                auto_guide(32), set_guide_refine(8)
  diagonal_refine16_hw64              set_guide(diagonal, 64), set_guide_refine(16)
Per row: seconds, the reads whose borders equal those of band 4093, the histogram of guide_rounds, the reads not converged, the
peak arena bytes; for the pre-pass rows also the seconds of auto_guide alone and of the align call alone. With the kernel's
register / LDS / scratch remarks of the build. Prints one JSON line and writes it to argv[1] (profiles/auto_guide/bench.json)."""
import json, os, re, subprocess, sys, tempfile, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_band_cases as gc
from dynamont_amd import Aligner, _native, synth

READS = int(os.environ.get("AG_READS", 128))
REPEATS = int(os.environ.get("AG_REPEATS", 3))
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn5.model"), 5, seed=7, stdev=0.25)
_, mean, sd = synth.read_model_file(model)
mean_code, sd_code = synth.code_order_table(mean, sd, gc.K, False)
rng = np.random.default_rng(20261019)
reads = [gc.make_read(rng, mean_code, sd_code, int(rng.integers(1800, 2201)), 6.0, stall=float(rng.uniform(0.3, 0.5))) for _ in range(READS)]
sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
true_guides = np.concatenate([gc.true_guide(r) for r in reads])
diagonals = np.concatenate([gc.diagonal(r) for r in reads])


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


def same(x, y):
    return sum(int(x.status[i] == 0 and y.status[i] == 0 and np.array_equal(borders(x, i), borders(y, i))) for i in range(READS))


al = Aligner(model, gc.PORE, band=400, device=0)
rec = {"workload": "%d stalled reads, %d samples, %d k-mers (syn5, dna_r9)" % (READS, sum(len(s) for s in sig), sum(r.n_kmers for r in reads)),
       "repeats": REPEATS}
widest = Aligner(model, gc.PORE, band=4093, device=0)
res_widest = widest.align_batch(sig, seq)
widest.close()
rec["band_4093_ok"] = int((res_widest.status == 0).sum())
extra = {}


def guided_job(hw, guide, refine):
    """guide None: the pre-pass makes it"""
    def run():
        with al.batch(sig, seq) as b:
            t0 = time.perf_counter()
            if guide is None:
                b.auto_guide(hw)
            else:
                b.set_guide(guide, hw)
            t1 = time.perf_counter()
            if refine > 1:
                b.set_guide_refine(refine)
            b.align(True)
            t2 = time.perf_counter()
            res = b.fetch()
            res.guide_rounds, res.guide_converged = b.guide_rounds()
            extra["arena"], extra["guide_s"], extra["align_s"] = b.arena_bytes(), t1 - t0, t2 - t1
            return res
    return run


def row(name, fn, rounds=True):
    res, s, every = timed(fn)
    r = {"seconds": round(s, 4), "seconds_all": [round(x, 4) for x in every], "reads_ok": int((res.status == 0).sum()),
         "reads_with_the_borders_of_band_4093": same(res, res_widest)}
    if rounds:
        r["guide_rounds"] = {str(int(k)): int(v) for k, v in zip(*np.unique(res.guide_rounds, return_counts=True))}
        r["not_converged"] = int(((res.guide_converged == 0) & (res.status == 0)).sum())
        r["peak_arena_bytes"] = int(extra["arena"])
        r["seconds_guide_call_last_run"] = round(extra["guide_s"], 4)
        r["seconds_align_call_last_run"] = round(extra["align_s"], 4)
    rec[name] = r
    print(name, json.dumps(r), flush=True)
    return res


row("plain_band_400", lambda: al.align_batch(sig, seq), rounds=False)
al.set_band_retry(1)
row("retry", lambda: al.align_batch(sig, seq), rounds=False)
al.set_band_retry(0)
al.set_band_margin(False)
row("guided_true_starts_hw64", guided_job(64, true_guides, 1))
row("prepass_1_hw64", guided_job(64, None, 1))
row("prepass_refine8_hw64", guided_job(64, None, 8))
row("prepass_refine8_hw32", guided_job(32, None, 8))
row("diagonal_refine16_hw64", guided_job(64, diagonals, 16))
# how far the pre-pass guide strays from the true-starts guide, in columns
for hw in (64, 32):
    with al.batch(sig, seq) as b:
        b.auto_guide(hw)
        stray = [int(np.abs(g.astype(np.int64) - gc.true_guide(r).astype(np.int64)).max()) for g, r in zip(b.guide(), reads)]
    rec["prepass_max_distance_from_true_starts_hw%d" % hw] = {"max": max(stray), "reads_above_hw_minus_8": int(sum(s > hw - 8 for s in stray))}
al.close()
# the kernel's resources as the build reports them (device code only, nothing is run)
cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                        "-x", "hip", os.path.join(_native.CSRC, "auto_guide.hip"), "-o", os.path.join(d, "ag.o")]
r = subprocess.run(cmd, capture_output=True, text=True)
res_lines, name = {}, None
for line in r.stderr.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        name = m.group(1)
        res_lines[name] = {}
    m = re.search(r"remark:\s+(VGPRs|AGPRs|SGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
    if m and name:
        res_lines[name][m.group(1)] = int(m.group(2))
rec["kernel_resources"] = res_lines
rec["kernel_resources_note"] = "LDS is dynamic: 2 rows of 2 hw + 4 doubles + 64 B per workgroup"
print(json.dumps(rec))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    json.dump(rec, open(sys.argv[1], "w"), indent=1)
