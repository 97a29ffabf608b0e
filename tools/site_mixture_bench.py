#!/usr/bin/env python
"""GPU box: what the per-site mixture fit on the device (Aligner.site_mixture) saves over the host route. One table of 2 x 2^20
sites with histograms (bins = 32 over [-4, 4)), both halves filled with seeded counters through Aligner.site_summary_add as
tools/site_compare_bench.py fills its own; in the second half one site in two carries a second cluster four bins up. Two wall times
over ONE window of 2^20 pairs, best of 3, each after its own warm-up:
  device   Aligner.site_mixture(0, 2^20, 2^20): the kernel, 80 bytes per pair back, the host's derived columns
  host     two site_histogram() fetches of 2^20 sites each plus the same fit vectorised in NumPy (fit_numpy below: the definition's
           operations and its summation tree on arrays, only the sites still running carried from round to round; np.exp, which
           is not the library's strict exp)
and whether both give the same status and iters, the largest relative difference of the parameters where they do, and the
distribution of iters and status. Prints one JSON line and writes it to argv[1] if given (profiles/site_mixture/cost.json).
--pairs N / --repeats R / --host-repeats R shrink the run (the JSON says so)."""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

BINS, LO, HI = 32, -4.0, 4.0
MAX_ITERS, TOL, MIN_N = 128, 1e-3, 8


def gsum(t, g=64):
    """the definition's tree: G partials (one counter each for Bc <= G), then partner sums -- lane 0's value is the pairwise tree"""
    p = np.zeros((t.shape[0], g), dtype=np.float64)
    p[:, :t.shape[1]] = t
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0]


def estep(x, mu0, mu1, var0, var1, pi0, pi1):
    a0, a1 = pi0 / np.sqrt(var0), pi1 / np.sqrt(var1)
    d0, d1 = x[None, :] - mu0[:, None], x[None, :] - mu1[:, None]
    q0, q1 = -0.5 * ((d0 * d0) / var0[:, None]), -0.5 * ((d1 * d1) / var1[:, None])
    qm = np.where(q1 > q0, q1, q0)
    p0, p1 = a0[:, None] * np.exp(q0 - qm), a1[:, None] * np.exp(q1 - qm)
    s = p0 + p1
    return p0 / s, p1 / s


def fit_numpy(a, b, chunk=1 << 16):
    """a, b: uint32 [n, BINS + 2]. The thirteen device columns (dict of arrays)."""
    n = a.shape[0]
    w = (HI - LO) / BINS
    vfloor, tol_mu = (w * w) / 12.0, TOL * w
    x = LO + (np.arange(BINS + 2, dtype=np.float64) - 0.5) * w
    out = {k: np.full(n, np.nan) for k in ("pi1", "mu0", "mu1", "var0", "var1", "r_a", "r_b")}
    out.update(n_a=a[:, 1:-1].sum(axis=1, dtype=np.uint64).astype(np.uint32), n_b=b[:, 1:-1].sum(axis=1, dtype=np.uint64).astype(np.uint32),
               out_a=a[:, 0] + a[:, -1], out_b=b[:, 0] + b[:, -1], iters=np.zeros(n, dtype=np.uint32), status=np.ones(n, dtype=np.uint32))
    for c0 in range(0, n, chunk):
        fa, fb = a[c0:c0 + chunk].astype(np.float64), b[c0:c0 + chunk].astype(np.float64)
        fa[:, 0] = fa[:, -1] = fb[:, 0] = fb[:, -1] = 0.0
        c = fa + fb
        with np.errstate(divide="ignore", invalid="ignore"):
            cnt = gsum(c)
            m = gsum(c * x) / cnt
            v = gsum(c * ((x - m[:, None]) * (x - m[:, None]))) / cnt
        idx = np.flatnonzero(~(cnt < MIN_N) & (v > vfloor))            # rows of the chunk that are fitted
        sd = np.sqrt(v[idx])
        P = [m[idx] - sd, m[idx] + sd, v[idx].copy(), v[idx].copy(), np.full(idx.size, 0.5), np.full(idx.size, 0.5)]
        status, iters = np.full(idx.size, 2, dtype=np.uint32), np.zeros(idx.size, dtype=np.uint32)
        live = np.arange(idx.size)                                      # positions in idx still running
        for it in range(1, MAX_ITERS + 1):
            if live.size == 0:
                break
            cl = c[idx[live]]
            mu0, mu1, var0, var1, pi0, pi1 = (p[live] for p in P)
            g0, g1 = estep(x, mu0, mu1, var0, var1, pi0, pi1)
            t0, t1 = cl * g0, cl * g1
            n0, n1 = gsum(t0), gsum(t1)
            dead = (n0 < 1.0) | (n1 < 1.0)
            with np.errstate(divide="ignore", invalid="ignore"):
                nm0, nm1 = gsum(t0 * x) / n0, gsum(t1 * x) / n1
                nv0 = gsum(t0 * ((x - nm0[:, None]) * (x - nm0[:, None]))) / n0
                nv1 = gsum(t1 * ((x - nm1[:, None]) * (x - nm1[:, None]))) / n1
                nv0, nv1 = np.where(vfloor > nv0, vfloor, nv0), np.where(vfloor > nv1, vfloor, nv1)
                tot = n0 + n1
                np0, np1 = n0 / tot, n1 / tot
                d0, d1 = np.abs(nm0 - mu0), np.abs(nm1 - mu1)
                done = (np.where(d1 > d0, d1, d0) <= tol_mu) & (np.abs(np1 - pi1) <= TOL) & ~dead
            keep = ~dead
            for p, new in zip(P, (nm0, nm1, nv0, nv1, np0, np1)):
                p[live[keep]] = new[keep]
            iters[live[keep]] = it
            status[live[dead]] = 3
            status[live[done]] = 0
            live = live[keep & ~done]
        g0, g1 = estep(x, *P)
        swap = P[0] > P[1]
        gs = np.where(swap[:, None], g0, g1)
        rows = c0 + idx
        out["r_a"][rows], out["r_b"][rows] = gsum(fa[idx] * gs), gsum(fb[idx] * gs)
        out["pi1"][rows] = np.where(swap, P[4], P[5])
        out["mu0"][rows], out["mu1"][rows] = np.where(swap, P[1], P[0]), np.where(swap, P[0], P[1])
        out["var0"][rows], out["var1"][rows] = np.where(swap, P[3], P[2]), np.where(swap, P[2], P[3])
        out["iters"][rows], out["status"][rows] = iters, status
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=None, help="default: --repeats")
    args = ap.parse_args()
    from dynamont_amd import Aligner, synth
    N = args.pairs
    host_repeats = args.repeats if args.host_repeats is None else args.host_repeats
    d = tempfile.mkdtemp()
    model = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
    al = Aligner(model, "rna004", device=0)
    al.set_site_summary(2 * N)
    al.set_site_histogram(BINS, LO, HI)
    rng = np.random.default_rng(12)
    edges = LO + np.arange(BINS + 1, dtype=np.float64) * ((HI - LO) / BINS)
    for half in range(2):
        # a site's rows spread over a few neighbouring bins around a centre of its own, as event means do; one site in 16 empty
        centre = rng.integers(4, BINS - 8, N)
        level = np.zeros((N, BINS + 2), dtype=np.uint32)
        for k in range(-3, 4):
            level[np.arange(N), centre + k] = rng.integers(0, 40, N) // (1 + abs(k))
        if half:                                                        # the second sample: one site in two has a modified share
            mod = np.flatnonzero(rng.random(N) < 0.5)
            for k in range(-2, 3):
                level[mod, centre[mod] + 4 + k] += (rng.integers(0, 30, mod.size) // (1 + abs(k))).astype(np.uint32)
        level[rng.random(N) < 1 / 16] = 0
        dwell = np.zeros((N, 16), dtype=np.uint32)
        rows = level.sum(axis=1).astype(np.uint64)
        zeros = np.zeros(N, dtype=object)
        al.site_summary_add(half * N, {"n_rows": rows, "n_samples": rows * np.uint64(10), "dwell_sq": rows * np.uint64(100), "M1": zeros, "M2": zeros},
                            {"level": level, "dwell": dwell, "edges": edges})

    def host_route(n=N):
        t0 = time.perf_counter()
        a, b = al.site_histogram(0, n)["level"], al.site_histogram(N, N + n)["level"]
        t_fetch = time.perf_counter() - t0
        return fit_numpy(a, b), time.perf_counter() - t0, t_fetch

    al.site_mixture(0, N, N)                                            # warm-up: the staging buffer, the kernel's first launch
    t_dev = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        got = al.site_mixture(0, N, N)
        t_dev.append(time.perf_counter() - t0)
    host_route(min(N, 1 << 16))                                         # warm-up (a sixteenth of the window: NumPy has no first-launch cost)
    t_host, t_fetch = [], []
    for _ in range(host_repeats):
        want, t, tf = host_route()
        t_host.append(t)
        t_fetch.append(tf)
    al.close()
    same = (got["status"] == want["status"]) & (got["iters"] == want["iters"])
    ints = all(np.array_equal(got[k], want[k]) for k in ("n_a", "n_b", "out_a", "out_b"))
    ok = same & (got["status"] != 1)
    rel = {}
    for k in ("pi1", "mu0", "mu1", "var0", "var1", "r_a", "r_b"):
        den = np.maximum(np.abs(want[k][ok]), 1e-300)
        rel[k] = float(np.max(np.abs(got[k][ok] - want[k][ok]) / den)) if ok.any() else None
    fitted = got["status"] != 1
    rec = {"window_pairs": N, "bins": BINS, "table_sites": 2 * N, "max_iters": MAX_ITERS, "tol": TOL, "min_n": MIN_N, "repeats": {"device": args.repeats, "host": host_repeats},
           "device_ms_best": round(1e3 * min(t_dev), 3), "device_ms": [round(1e3 * t, 3) for t in t_dev],
           "host_ms_best": round(1e3 * min(t_host), 1), "host_ms": [round(1e3 * t, 1) for t in t_host],
           "of_which_two_fetches_ms": round(1e3 * min(t_fetch), 3), "ratio_host_over_device": round(min(t_host) / min(t_dev), 1),
           "status_counts": {str(s): int((got["status"] == s).sum()) for s in range(4)},
           "iters_of_fitted_pairs": {"mean": round(float(got["iters"][fitted].mean()), 2), "median": int(np.median(got["iters"][fitted])),
                                     "p90": int(np.percentile(got["iters"][fitted], 90)), "max": int(got["iters"].max())},
           "same_status_and_iters": bool(same.all()), "pairs_with_other_status_or_iters": int((~same).sum()), "same_counts": bool(ints),
           "largest_relative_difference_where_same": rel, "bytes_back_per_pair": {"device": 80, "host": 2 * 4 * (BINS + 18)}}
    print(json.dumps(rec))
    if args.out:
        json.dump(rec, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
