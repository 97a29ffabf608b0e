"""Shared by tests/test_auto_guide_host.py and tests/test_gpu_auto_guide.py (no GPU, no library): the two definitions of the
self-guided band restated in plain NumPy float64 -- the pre-pass of dyn_batch_auto_guide and the
refinement of dyn_batch_set_guide_refine, the latter over ``guided_band_cases.model_align`` --, the g++ build of the pre-pass
(tests/device_math/auto_guide_host.cpp over dynamont_amd/csrc/auto_guide_kernels.hpp) and the small synthetic reads of the
edge cases. The read families are those of ``guided_band_cases.build_reads``."""
import ctypes as C
import os
import subprocess

import numpy as np

import guided_band_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamont_amd", "csrc")
NEG = -np.inf
HALF_LOG_2PI = float.fromhex("0x1.d67f1c864beb4p-1")   # dp_math.hpp


def score_row(x, mean, sd, nls):
    """log_normal_pdf_strict, operation by operation"""
    z = (x - mean) / sd
    return (((-0.5 * z) * z) + nls) - HALF_LOG_2PI


def prepass_guide(signal, mean, sd, nls, log_m1, log_e2, hw):
    """the pre-pass: mean / sd / nls are the emission entries of lattice columns 1 .. N-1 (entry n - 1). Returns the int32
    guide, one entry per sample. Whole rows in absolute columns; everything outside a row's window is -inf."""
    x = np.asarray(signal, dtype=np.float64)
    T, N = len(x) + 1, len(mean) + 1
    hw = int(hw)
    vE, vM = np.full(N, NEG), np.full(N, NEG)
    vE[0] = 0.0
    c, w_lo, w_hi = 0, 0, 1
    guide = np.zeros(T - 1, dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(1, T):
            e, m = vE[w_lo:w_hi], vM[w_lo:w_hi]
            s = np.where(m < e, e, m)
            valid = s > NEG                                         # a NaN never enters
            a = c
            if valid.any():
                a = w_lo + int(np.flatnonzero(valid & (s == s[valid].max()))[0])
            lo = max(0, N - 1 - (T - 1 - t) // 2)
            hi = min(N - 1, (t + 1) // 2)
            c = min(max(c, a, lo), hi)
            guide[t - 1] = c
            a0, b0 = max(c - hw, 1), min(c + hw + 1, N)
            nE, nM = np.full(N, NEG), np.full(N, NEG)
            if a0 < b0:
                n = np.arange(a0, b0)
                sc = score_row(x[t - 1], mean[n - 1], sd[n - 1], nls[n - 1])
                nM[n] = (vE[n - 1] + sc) + log_m1
                p, q = (vM[n] + sc) + 0.0, (vE[n] + sc) + log_e2
                nE[n] = np.where(p < q, q, p)
            vE, vM = nE, nM
            w_lo, w_hi = a0, max(a0, b0)
    return guide


def next_guide(mo):
    """g'[s] = the called path's column at lattice row s + 1 (0 before the first border)"""
    return mo.pathn[1:].astype(np.int32)


def refine(signal, mean, sd, log_m1, log_e2, guide, hw, max_rounds):
    """the refinement over model_align. Returns (rounds, converged, final guide, the last alignment, Z of every alignment)"""
    g = np.asarray(guide, dtype=np.int32).copy()
    zs = []
    mo = None
    for r in range(int(max_rounds)):
        mo = gc.model_align(signal, mean, sd, log_m1, log_e2, g, hw)
        if not mo.ok:
            return r + 1, 0, g, mo, zs
        zs.append(mo.Z)
        g2 = next_guide(mo)
        if np.array_equal(g2, g):
            return r + 1, 1, g, mo, zs
        if r + 1 < max_rounds:
            g = g2
    return int(max_rounds), 0, g, mo, zs


def guide_invariants(g, n_columns):
    """non-decreasing, within [0, N - 1], connecting the corners (the last row is centred on column N - 1)"""
    g = np.asarray(g, dtype=np.int64)
    return bool(g.size == 0 or ((np.diff(g) >= 0).all() and g[0] >= 0 and g[-1] == n_columns - 1))


# ------------------------------------------------------------------------------------------------------- the g++ build
def build_host(outdir):
    so = os.path.join(str(outdir), "libag_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "device_math", "auto_guide_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.ag_host_guide.restype = C.c_int
    return lib


def host_guide(lib, signal, mean, sd, nls, log_m1, log_e2, hw):
    x = np.ascontiguousarray(signal, dtype=np.float64)
    mean, sd, nls = (np.ascontiguousarray(v, dtype=np.float64) for v in (mean, sd, nls))
    g = np.zeros(len(x), dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.ag_host_guide(C.c_int(len(x) + 1), C.c_int(len(mean) + 1), C.c_int(int(hw)), p(x), p(mean), p(sd), p(nls),
                           C.c_double(log_m1), C.c_double(log_e2), p(g))
    assert rc == 0
    return g


# ------------------------------------------------------------------------------------------------------- edge-case reads
def edge_reads(mean_code, sd_code):
    """name -> read (guided_band_cases.make_read): N = 2; T = 2 (N - 1) + 1, where lo == hi in every row; a NaN sample"""
    rng = np.random.default_rng(7100)
    out = {"n2": gc.make_read(rng, mean_code, sd_code, 1, 9.0)}
    r = gc.make_read(rng, mean_code, sd_code, 40, 1.0)
    while len(r.signal) != 2 * r.n_kmers:                           # dwell max(2, Poisson(0.05)): 2 samples per k-mer
        r = gc.make_read(rng, mean_code, sd_code, 40, 0.05)
    out["tight"] = r
    r = gc.make_read(rng, mean_code, sd_code, 50, 6.0)
    r.signal[len(r.signal) // 3] = np.nan
    out["nan"] = r
    return out
