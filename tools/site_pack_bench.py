#!/usr/bin/env python
"""GPU box: what moving the per-site table by content (Aligner.site_table_pack / site_summary_merge) saves over the routes by id
window. One process, histograms of 32 bins over [-4, 4), seeded records, every wall time the best of `--repeat` after a warm-up:
  dense    a table of --dense-sites sites (default 10^8) with --live (default 4 * 10^6) scattered live sites
           pack    site_table_pack()                                        against
           windows every 2^20-id window: site_summary + site_histogram + flatnonzero(n_rows) (utils.save_site_table's default route)
  sparse   a map of --capacity rows (default 5 * 10^7) at load 0.5 over an id space of 4 * 10^9
           pack    site_table_pack()                                        against
           windows site_map_windows(20), then the same per occupied window
  merge    --live scattered records into an empty dense table
           keyed   site_summary_merge(packed)                               against
           windows site_summary_add over the 2^20-id windows that hold them (utils.load_site_control's route)
and that each pair of routes gives the same integers. Prints one JSON line; with --out the cases of this run are written into
that file beside the cases an earlier run left there (profiles/site_pack/cost.json: dense and merge at full size, sparse at
--scale 64), each with its own `scale` and `repeat`. `--scale F` divides every size, the sparse id space included, by F (the windows routes move
256 bytes per id of every window they touch: at full size the sparse one alone moves about a terabyte)."""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from dynamont_amd import Aligner, synth

ap = argparse.ArgumentParser()
ap.add_argument("--dense-sites", type=int, default=100_000_000)
ap.add_argument("--live", type=int, default=4_000_000)
ap.add_argument("--capacity", type=int, default=50_000_000)
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--repeat", type=int, default=2)
ap.add_argument("--skip", default="", help="comma list of dense, sparse, merge")
ap.add_argument("--out", default="")
args = ap.parse_args()
DENSE, LIVE, CAP = (max(1 << 12, int(v / args.scale)) for v in (args.dense_sites, args.live, args.capacity))
BINS, LO, HI = 32, -4.0, 4.0
STEP = 1 << 20
edges = LO + np.arange(BINS + 1, dtype=np.float64) * ((HI - LO) / BINS)
d = tempfile.mkdtemp()
model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)


def records(rng, n, id_space):
    """n records of distinct sorted ids below id_space: a covered site's words and counters"""
    ids = np.unique(rng.integers(0, id_space, int(n * 1.1), dtype=np.uint64))[:n]
    rows = rng.integers(1, 60, ids.size).astype(np.uint64)
    level = np.zeros((ids.size, BINS + 2), dtype=np.uint32)
    centre = rng.integers(2, BINS - 2, ids.size)
    level[np.arange(ids.size), centre] = rows.astype(np.uint32)
    dwell = np.zeros((ids.size, 16), dtype=np.uint32)
    dwell[:, 3] = rows.astype(np.uint32)
    limbs = [rows, rows * np.uint64(9), rows * np.uint64(81), rng.integers(0, 1 << 62, ids.size, dtype=np.uint64), np.zeros(ids.size, dtype=np.uint64),
             rng.integers(0, 1 << 62, ids.size, dtype=np.uint64), np.zeros(ids.size, dtype=np.uint64)]
    return {"site": ids, "limbs": limbs, "level": level, "dwell": dwell, "edges": edges, "totals": None}


def best(fn, repeat=args.repeat):
    fn()
    out, t = None, []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return out, min(t)


def by_windows(al, num_sites, windows=None):
    """the covered sites through windows of ids: what utils.save_site_table does by default"""
    site, limbs, level, dwell = [], [[] for _ in range(7)], [], []
    starts = range(0, num_sites, STEP) if windows is None else [int(w) * STEP for w in windows]
    for w0 in starts:
        w1 = min(w0 + STEP, num_sites)
        s = al.site_summary(w0, w1)
        idx = np.flatnonzero(s["n_rows"])
        h = al.site_histogram(w0, w1)
        site.append(idx.astype(np.uint64) + np.uint64(w0))
        for f in range(7):
            limbs[f].append(s["limbs"][f][idx])
        level.append(h["level"][idx])
        dwell.append(h["dwell"][idx])
    return {"site": np.concatenate(site), "limbs": [np.concatenate(c) for c in limbs], "level": np.concatenate(level), "dwell": np.concatenate(dwell)}


def same(a, b):
    return bool(np.array_equal(a["site"], b["site"]) and all(np.array_equal(x, y) for x, y in zip(a["limbs"], b["limbs"]))
                and np.array_equal(a["level"], b["level"]) and np.array_equal(a["dwell"], b["dwell"]))


def handle(num_sites, capacity=None):
    al = Aligner(model, "rna004", device=0)
    al.set_site_summary(num_sites, capacity=capacity)
    al.set_site_histogram(BINS, LO, HI)
    return al


out = {"bins": BINS, "scale": args.scale, "repeat": args.repeat}
rng = np.random.default_rng(30)
skip = set(args.skip.split(","))
if "dense" not in skip or "merge" not in skip:
    rec = records(rng, LIVE, DENSE)
    al = handle(DENSE)
    _, t_keyed_first = best(lambda: al.site_summary_merge(rec), repeat=1)      # (warm-up + one timed: the table holds the records twice)
    al.reset_site_summary()
    t0 = time.perf_counter()
    al.site_summary_merge(rec)
    t_keyed = time.perf_counter() - t0
    if "dense" not in skip:
        packed, t_pack = best(al.site_table_pack)
        wins, t_win = best(lambda: by_windows(al, DENSE), repeat=1)
        out["dense"] = {"sites": DENSE, "live": int(rec["site"].size), "record_bytes": 60 + 4 * (BINS + 18), "pack_s": round(t_pack, 4),
                        "windows_s": round(t_win, 4), "ratio": round(t_win / t_pack, 2), "same_integers": same(packed, wins),
                        "bytes_over_pcie_pack": int(rec["site"].size) * (60 + 4 * (BINS + 18)), "bytes_over_pcie_windows": DENSE * (56 + 4 * (BINS + 18))}
    if "merge" not in skip:
        al.reset_site_summary()

        def add_windows():
            site = rec["site"].astype(np.int64)
            for w0 in np.unique(site // STEP).tolist():
                w0 *= STEP
                w1 = min(w0 + STEP, DENSE)
                a, b = np.searchsorted(site, [w0, w1])
                rel = site[a:b] - w0
                cols = {}
                for k, f in (("n_rows", 0), ("n_samples", 1), ("dwell_sq", 2)):
                    cols[k] = np.zeros(w1 - w0, dtype=np.uint64)
                    cols[k][rel] = rec["limbs"][f][a:b]
                for k, f in (("M1", 3), ("M2", 5)):
                    cols[k] = np.zeros(w1 - w0, dtype=object)
                    cols[k][rel] = [int(v) for v in rec["limbs"][f][a:b]]
                hist = {"level": np.zeros((w1 - w0, BINS + 2), dtype=np.uint32), "dwell": np.zeros((w1 - w0, 16), dtype=np.uint32), "edges": edges}
                hist["level"][rel] = rec["level"][a:b]
                hist["dwell"][rel] = rec["dwell"][a:b]
                al.site_summary_add(w0, cols, hist)

        t0 = time.perf_counter()
        add_windows()
        t_add = time.perf_counter() - t0
        out["merge"] = {"records": int(rec["site"].size), "sites": DENSE, "keyed_s": round(t_keyed, 4), "windows_s": round(t_add, 4),
                        "ratio": round(t_add / t_keyed, 2), "same_integers": same(al.site_table_pack(), rec)}
    al.close()
if "sparse" not in skip:
    ID_SPACE = max(CAP, int(4_000_000_000 / args.scale))
    rec = records(rng, CAP // 2, ID_SPACE)
    al = handle(ID_SPACE, CAP)
    t0 = time.perf_counter()
    al.site_summary_merge(rec)
    t_fill = time.perf_counter() - t0
    packed, t_pack = best(al.site_table_pack, repeat=1)
    t0 = time.perf_counter()
    windows = al.site_map_windows(20)
    wins = by_windows(al, ID_SPACE, windows.tolist())
    t_win = time.perf_counter() - t0
    m = al.site_map()
    out["sparse"] = {"capacity": CAP, "id_space": ID_SPACE, "keys": m["n_keys"], "sites_dropped": m["sites_dropped"], "fill_keyed_s": round(t_fill, 4), "pack_s": round(t_pack, 4),
                     "windows_s": round(t_win, 4), "occupied_windows": int(windows.size), "ratio": round(t_win / t_pack, 2),
                     "same_integers": same(packed, wins)}
    al.close()
for case in ("dense", "merge", "sparse"):  # every case says at what size it ran
    if case in out:
        out[case].update(scale=args.scale, repeat=args.repeat)
out = {k: v for k, v in out.items() if k not in ("scale", "repeat")}
print(json.dumps(out))
if args.out:  # the cases of this run into the file, beside those an earlier run (another --scale, another --skip) left there
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    kept = json.load(open(args.out)) if os.path.exists(args.out) else {}
    kept.update(out)
    kept["tool"] = "tools/site_pack_bench.py: wall seconds in one process on one MI355X; `scale` divides the planned sizes"
    open(args.out, "w").write(json.dumps(kept, indent=1) + "\n")
