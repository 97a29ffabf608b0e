#!/usr/bin/env python
"""GPU box: what the posterior-weighted per-base levels (Aligner.set_soft_levels) cost on the async align line. cfg2's shape
(1 024 reads x ~20 k samples, syn9, band 400) through align_async in steady state (DEPTH tickets in flight), three kinds of
ticket alternating every ROUND batches in one process, BATCHES of each after a warm-up: the switch off ("off"), the soft levels
("soft") and, as the yardstick with the same lane mapping, the credible intervals at mass 0.9 ("interval"). Prints one JSON line
(Msamp/s for each, the ratios against "off", ms per batch, per kind the means of dyn_batch_timing's ms_dp -- the read queue --
and ms_trace -- its traceback, mpost and lattice-phase share plus the per-segment kernels; the phase is what they grow by -- and
each phase's share of its own batch) and merges it into the JSON file argv[1] if given (default profiles/soft_levels/cost.json;
the other keys it holds are kept).

Two effects are mixed in the plain run: the phase itself, and that such a ticket takes one launch per batch instead of the
resident session. Run it a second time with DYN_NO_SESSION=1 in the environment: "off" then takes one launch per batch as well,
the record goes under "align_line_no_session", and the ratios show the phase alone.

  soft_levels_bench.py [out.json]             the align line, off / soft / interval
  soft_levels_bench.py listing [csrc] [out]   one line per kernel of every .hip file under csrc (default: this tree's
                                              dynamont_amd/csrc) with hipcc's resource-usage remarks -- run on two trees
                                              and compare (profiles/soft_levels/kernel_resources.txt); needs no GPU
"""
import hashlib, json, os, re, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "soft_levels", "cost.json")


def merge(path, rec):
    old = json.load(open(path)) if os.path.exists(path) else {}
    old.update(rec)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(old, open(path, "w"), indent=1)
    print(json.dumps(rec))


def listing(csrc):
    """['file  kernel  sgpr=.. vgpr=.. ...'] of every kernel of every .hip file in csrc, sorted"""
    from concurrent.futures import ThreadPoolExecutor
    from dynamont_amd import _native
    keys = (("sgpr", r"TotalSGPRs: (\d+)"), ("vgpr", r"\bVGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"),
            ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
            ("sspill", r"SGPRs Spill: (\d+)"), ("vspill", r"VGPRs Spill: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"))

    def one(src):
        cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-Rpass-analysis=kernel-resource-usage", "-I", csrc, "-x", "hip", "-c",
                                                                os.path.join(csrc, src), "-o", os.devnull]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
        out, cur = [], None
        for line in text.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                mangled = m.group(1)
                name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
                name = re.sub(r"\(.*$", "", name).replace("void ", "").replace("dynk::", "").replace("(anonymous namespace)::", "")
                if len(name) > 90:
                    name = name[:80] + "...#" + hashlib.sha1(mangled.encode()).hexdigest()[:8]
                cur = {"name": name}
                out.append(cur)
            for key, pat in keys:
                m = re.search(pat, line)
                if m and cur is not None:
                    cur[key] = int(m.group(1))
        return ["%s  %s  %s" % (src, k["name"], " ".join("%s=%d" % (key, k.get(key, -1)) for key, _ in keys)) for k in out]
    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    with ThreadPoolExecutor(max_workers=4) as ex:
        return sorted(line for lines in ex.map(one, srcs) for line in lines)


if len(sys.argv) > 1 and sys.argv[1] == "listing":
    from dynamont_amd import _native
    lines = listing(sys.argv[2] if len(sys.argv) > 2 else _native.CSRC)
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 3:
        open(sys.argv[3], "w").write(text)
    else:
        sys.stdout.write(text)
    sys.exit(0)

from dynamont_amd import Aligner, synth

BATCHES = int(os.environ.get("SL_BATCHES", 16))
ROUND = int(os.environ.get("SL_ROUND", 4))
DEPTH = int(os.environ.get("SL_DEPTH", 4))
NO_SESSION = os.environ.get("DYN_NO_SESSION", "") not in ("", "0")
MASS = 0.9
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
_, mean, sd = synth.read_model_file(model)
cfg = synth.CONFIGS["cfg2"]
reads = [synth.make_reads(cfg["seed"] + j, 1024, cfg["pore"], mean, sd, cfg["n_bases"]) for j in range(2)]
packed = [synth.pack_reads(r) for r in reads]
samples = [int(p[1][-1]) for p in packed]
al = Aligner(model, cfg["pore"], band=400, device=0)


KINDS = ("off", "soft", "interval")


def switch(kind):
    al.set_border_interval(0)
    al.set_soft_levels(False)
    if kind == "interval":
        al.set_border_interval(MASS)
    elif kind == "soft":
        al.set_soft_levels(True)


def run(kind, n):
    """n batches of `kind`, DEPTH in flight; (samples, wall time from the first submit to the last wait, sum of the tickets'
    ms_trace, tickets that took a launch of their own, sum of ms_dp)"""
    switch(kind)
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


for c in KINDS:
    run(c, 6)   # warm-up: buffers of every kind cached
tot = {c: [0, 0.0, 0.0, 0, 0, 0.0] for c in KINDS}
for r in range(BATCHES // ROUND):
    for c in KINDS if r % 2 == 0 else KINDS[::-1]:
        s, dt, tr, ln, dp = run(c, ROUND)
        tot[c][0] += s
        tot[c][1] += dt
        tot[c][2] += tr
        tot[c][3] += ln
        tot[c][4] += ROUND
        tot[c][5] += dp
switch("off")
rate = {c: tot[c][0] / tot[c][1] / 1e6 for c in KINDS}
ms = {c: 1e3 * tot[c][1] / tot[c][4] for c in KINDS}
sweep_rows = sum(sum(len(x.signal) for x in r) for r in reads) / 2
rec = {"workload": "cfg2 (1024 reads x ~20 k samples, syn9, band 400), align_async, %d in flight" % DEPTH,
       "no_session": NO_SESSION, "batches_each": BATCHES, "mass": MASS,
       "msamp_s": {c: round(rate[c], 1) for c in KINDS},
       "ratio_to_off": {c: round(rate[c] / rate["off"], 4) for c in KINDS},
       "ms_per_batch": {c: round(ms[c], 3) for c in KINDS},
       "ms_trace_per_batch": {c: round(tot[c][2] / tot[c][4], 4) for c in KINDS},
       "ms_dp_per_batch": {c: round(tot[c][5] / tot[c][4], 4) for c in KINDS},
       # what a batch grows by against "off", and that as a share of the batch itself
       "phase_ms_per_batch": {c: round(ms[c] - ms["off"], 3) for c in KINDS[1:]},
       "phase_share_of_batch": {c: round((ms[c] - ms["off"]) / ms[c], 4) for c in KINDS[1:]},
       "rows_visited_per_batch": "%d rows walked by one wave each, 448 slots wide (both phases)" % sweep_rows,
       "ns_per_wave_row": {c: round(1e6 * (ms[c] - ms["off"]) / sweep_rows, 3) for c in KINDS[1:]},
       "tickets_with_a_launch_of_their_own": {c: "%d of %d" % (tot[c][3], tot[c][4]) for c in KINDS}}
merge(sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT, {"align_line_no_session" if NO_SESSION else "align_line": rec})
al.close()
