#!/usr/bin/env python
"""GPU box: what the per-border segment scores (Aligner.set_segment_scores) cost on the async align line. cfg2's shape (1 024
reads x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), the switch alternating
off / W = 8 / W = 64 every ROUND batches in one process, BATCHES of each after a warm-up; prints one JSON line (Msamp/s for
each, the ratios) and merges it into the JSON file argv[1] if given (default profiles/segment_scores/segment_scores_cost.json
keeps the other keys it holds: the kernels' resources, their traced times, the bench.py headline numbers).

  segment_scores_bench.py [out.json]            the align line, off / on
  segment_scores_bench.py resources [out.json]  LDS / VGPR / scratch of the compiled kernels (hipcc's resource-usage remarks;
                                                needs no GPU)
  segment_scores_bench.py trace STATS.csv [out.json]
                                                ms per batch of the new kernels beside k_event_short / k_median, from the
                                                kernel-stats CSV of ONE `rocprofv3 --kernel-trace --stats -- python
                                                tools/segment_scores_bench.py traced` run (event stats and scores W = 8 on)
  segment_scores_bench.py traced                the workload of that run: TRACED_BATCHES batches, both switches on
  segment_scores_bench.py traced-off            the same with both switches off: the trace must list none of the new kernels
"""
import csv, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "segment_scores", "segment_scores_cost.json")
NEW_KERNELS = ("k_score_window", "k_score_homog", "k_score_long")
TRACED_BATCHES = int(os.environ.get("SC_TRACED_BATCHES", 8))


def merge(path, rec):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(rec)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1)
    print(json.dumps(rec))


mode = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1] in ("resources", "trace", "traced", "traced-off") else ""

if mode == "resources":
    from dynamont_amd import _native
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c",
                                                            os.path.join(_native.CSRC, "segment_scores.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    res, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip().split("(")[0] or m.group(1)
            name = name.replace("void ", "").replace("dynk::", "")
            res[name] = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"AGPRs: (\d+)"), ("sgprs", r"SGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds_bytes_per_block", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res[name][key] = int(m.group(1))
    merge(sys.argv[2] if len(sys.argv) > 2 else DEFAULT_OUT,
          {"kernel_resources": res, "resident_budget": "about 13 KB of LDS and 152 VGPRs per lane beside a resident workgroup (DESIGN section 4)"})
    sys.exit(0)

if mode == "trace":
    per = {}
    for row in csv.DictReader(open(sys.argv[2])):
        name = row.get("Name") or row.get("KernelName") or ""
        for k in NEW_KERNELS + ("k_event_short", "k_event_long", "k_median(", "k_median_long", "k_final"):
            if k in name:
                key = k.rstrip("(")
                e = per.setdefault(key, {"calls": 0, "total_ms": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ms"] += float(row["TotalDurationNs"]) / 1e6
    for e in per.values():
        e["ms_per_batch"] = round(e["total_ms"] / TRACED_BATCHES, 4)
        e["total_ms"] = round(e["total_ms"], 3)
    merge(sys.argv[3] if len(sys.argv) > 3 else DEFAULT_OUT,
          {"kernel_trace": {"workload": "cfg2, %d batches, event stats and segment scores W = 8 on (one rocprofv3 --kernel-trace --stats run)" % TRACED_BATCHES,
                            "kernels": per}})
    sys.exit(0)

from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("SC_BATCHES", 24))
ROUND = int(os.environ.get("SC_ROUND", 4))
DEPTH = int(os.environ.get("SC_DEPTH", 4))
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
packed = [synth.pack_reads(synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"])) for j in range(2)]
samples = [int(p[1][-1]) for p in packed]
al = Aligner(model, cfg["pore"], band=400, device=0)


def run(window, n):
    """n batches with the window `window` (0 = off), DEPTH in flight; wall time from the first submit to the last wait"""
    al.set_segment_scores(window)
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


if mode in ("traced", "traced-off"):
    on = mode == "traced"
    al.set_event_stats(on)
    run(8 if on else 0, TRACED_BATCHES)
    al.close()
    sys.exit(0)

WINDOWS = (0, 8, 64)
for w in WINDOWS:
    run(w, 8)   # warm-up: buffers of every kind cached
tot = {w: [0, 0.0] for w in WINDOWS}
for r in range(BATCHES // ROUND):
    for w in WINDOWS if r % 2 == 0 else WINDOWS[::-1]:
        s, dt = run(w, ROUND)
        tot[w][0] += s
        tot[w][1] += dt
rate = {w: tot[w][0] / tot[w][1] / 1e6 for w in WINDOWS}
rec = {"align_line": {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight" % DEPTH,
                      "batches_each": BATCHES, "msamp_s_off": round(rate[0], 1), "msamp_s_w8": round(rate[8], 1),
                      "msamp_s_w64": round(rate[64], 1), "ratio_w8_off": round(rate[8] / rate[0], 4),
                      "ratio_w64_off": round(rate[64] / rate[0], 4)}}
merge(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT, rec)
al.close()
