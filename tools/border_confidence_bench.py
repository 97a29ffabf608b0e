#!/usr/bin/env python
"""GPU box: what the per-border posterior confidence (Aligner.set_border_confidence) costs on the async align line. cfg2's shape
(1 024 reads x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), the window
alternating 0 / 2 / 8 / 64 / 256 every ROUND batches in one process, BATCHES of each after a warm-up; prints one JSON line
(Msamp/s for each, the ratios against W = 0, and per window the means of dyn_batch_timing's ms_dp -- the read queue -- and
ms_trace -- its traceback, mpost and border-phase share plus the per-segment kernels; the phase is what they grow by) and merges it
into the JSON file argv[1] if given (default
profiles/border_confidence/cost.json; the other keys it holds are kept).

Two effects are mixed in the plain run: the phase itself, and that a ticket with W > 0 takes one launch per batch instead of the
resident session. Run it a second time with DYN_NO_SESSION=1 in the environment: W = 0 then takes one launch per batch as well,
the record goes under "align_line_no_session", and the ratios show the phase alone.

  border_confidence_bench.py [out.json]            the align line, W = 0 / 2 / 8 / 64 / 256
  border_confidence_bench.py resources [out.json]  registers / LDS / scratch of the launches that carry the phase (hipcc's
                                                   resource-usage remarks; needs no GPU)
"""
import json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "border_confidence", "cost.json")


def merge(path, rec):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(rec)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1)
    print(json.dumps(rec))


if len(sys.argv) > 1 and sys.argv[1] == "resources":
    from dynamont_amd import _native
    res = {}
    for src in ("nt_kernels.hip", "band_reads.hip"):
        cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
                                                                os.path.join(_native.CSRC, src), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        name = None
        for line in text.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0] or m.group(1)
                name = name.replace("void ", "").replace("dynk::", "")
                # k_read_queue<9 | 10, .>: JOB_ALIGN | JOB_BORDER, JOB_ALIGN_INPLACE | JOB_BORDER
                keep = "k_band_reads<DiagonalWindow, 256, 16, true, false, true>" in name or re.search(r"k_read_queue<(9|10),", name)
                name = name if keep else None
                if name:
                    res[name] = {}
            for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                             ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                             ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
                m = re.search(pat, line)
                if m and name:
                    res[name][key] = int(m.group(1))
    merge(sys.argv[2] if len(sys.argv) > 2 else DEFAULT_OUT, {"kernel_resources": res})
    sys.exit(0)

from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("BC_BATCHES", 24))
ROUND = int(os.environ.get("BC_ROUND", 4))
DEPTH = int(os.environ.get("BC_DEPTH", 4))
NO_SESSION = os.environ.get("DYN_NO_SESSION", "") not in ("", "0")
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"])) for j in range(2)]
samples = [int(p[1][-1]) for p in packed]
al = Aligner(model, cfg["pore"], band=400, device=0)


def run(window, n):
    """n batches with the window `window` (0 = off), DEPTH in flight; (samples, wall time from the first submit to the last
    wait, sum of the tickets' ms_trace, tickets that took a launch of their own)"""
    al.set_border_confidence(window)
    t0 = time.perf_counter()
    inflight, done, trace, launched, dp = [], 0, 0.0, 0, 0.0

    def finish(t, k):
        nonlocal done, trace, launched, dp
        t.wait()
        tm = t.timing()
        trace += tm["ms_trace"]
        dp += tm["ms_dp"]
        launched += tm["launches"] > 0
        t.close()
        done += samples[k]
    for j in range(n):
        inflight.append((al.align_async(*packed[j % 2], True), j % 2))
        if len(inflight) >= DEPTH:
            finish(*inflight.pop(0))
    for t, k in inflight:
        finish(t, k)
    return done, time.perf_counter() - t0, trace, launched, dp


WINDOWS = (0, 2, 8, 64, 256)
for w in WINDOWS:
    run(w, 8)   # warm-up: buffers of every kind cached
tot = {w: [0, 0.0, 0.0, 0, 0, 0.0] for w in WINDOWS}
for r in range(BATCHES // ROUND):
    for w in WINDOWS if r % 2 == 0 else WINDOWS[::-1]:
        s, dt, tr, ln, dp = run(w, ROUND)
        tot[w][5] += dp
        tot[w][0] += s
        tot[w][1] += dt
        tot[w][2] += tr
        tot[w][3] += ln
        tot[w][4] += ROUND
rate = {w: tot[w][0] / tot[w][1] / 1e6 for w in WINDOWS}
rec = {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight" % DEPTH,
       "no_session": NO_SESSION, "batches_each": BATCHES,
       "msamp_s": {"w%d" % w: round(rate[w], 1) for w in WINDOWS},
       "ratio_to_w0": {"w%d" % w: round(rate[w] / rate[0], 4) for w in WINDOWS},
       "ms_per_batch": {"w%d" % w: round(1e3 * tot[w][1] / tot[w][4], 3) for w in WINDOWS},
       "ms_trace_per_batch": {"w%d" % w: round(tot[w][2] / tot[w][4], 4) for w in WINDOWS},
       "ms_dp_per_batch": {"w%d" % w: round(tot[w][5] / tot[w][4], 4) for w in WINDOWS},
       "tickets_with_a_launch_of_their_own": {"w%d" % w: "%d of %d" % (tot[w][3], tot[w][4]) for w in WINDOWS}}
merge(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT, {"align_line_no_session" if NO_SESSION else "align_line": rec})
al.close()
