"""Shared by tests/test_guide_rescue_host.py and the GPU tests of the guide rescue (no GPU; the library only where a function takes it as an argument): the selection rule of
dyn_aligner_set_guide_rescue restated in Python ints, the g++ build of the product's rule (tests/device_math/guide_rescue_host.cpp
over dynamont_amd/csrc/guide_rescue_kernels.hpp), and what the CPU says about the fixture -- ``guided_band_cases.build_reads`` on
conftest's ``syn5`` table, pore ``dna_r9``, band 50. tests/test_guide_rescue_host.py recomputes every pinned value below from the
CPU oracle, ``band_margin_cases.brute`` and the NumPy chain of ``auto_guide_cases``; the GPU tests take their expectations from
here."""
import ctypes as C
import os
import subprocess

import numpy as np

import guided_band_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dynamont_amd", "csrc")
NONE = 0xFFFFFFFF
BAND = gc.STALL_BAND

# ---- the fixture, as the CPU sees it ----------------------------------------------------------------------------------------
A_MIN_MARGIN = 18            # family a (24 reads): every margin >= 18, and all 24 carry the borders of band 4093 already
B_MIN_MARGIN = 14            # family b (16 reads): every margin >= 14
STALL_FLAGGED_M1 = (1, 2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 15)   # stall reads with min(low, high) < 1
STALL_UNFLAGGED_M1 = {0: 2, 8: 1, 9: 5, 14: 1}                 # ... the other four and their minimum margins
M_ALL = 12                   # flags all 16 stall reads and still none of a or b
# the chain at half width 2, refine 8, over STALL_FLAGGED_M1 (in that order): alignments per read; read 4 does not converge
CHAIN_HW2_ROUNDS = (4, 6, 2, 8, 2, 2, 3, 2, 2, 3, 3, 2)
CHAIN_HW2_OPEN = (4,)
CHAIN_HW16_ROUNDS = 2        # at half width 16, refine 8, every stall read converges at alignment 2 (borders of band 4093)


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def decide(status, N, T, low, high, min_margin, max_T):
    """0 not flagged, 1 flagged and to be rescued, 2 flagged but T above max_T. A margin of NONE counts as +infinity."""
    if status != 0 or N < 2:
        return 0
    m = min(float("inf") if low == NONE else low, float("inf") if high == NONE else high)
    if not m < min_margin:
        return 0
    return 1 if T <= max_T else 2


def select(T, N, read, status, low, high, min_margin, max_T):
    """(code per read, list of descriptor indices in descriptor order) over a descriptor table"""
    code = np.zeros(len(status), dtype=np.uint8)
    lst = []
    for k in range(len(T)):
        r = int(read[k])
        c = decide(int(status[r]), int(N[k]), int(T[k]), int(low[r]), int(high[r]), int(min_margin), int(max_T))
        if c:
            code[r] = c
        if c == 1:
            lst.append(k)
    return code, lst


def build_host(outdir):
    so = os.path.join(str(outdir), "libgr_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, "-o", so,
                    os.path.join(ROOT, "tests", "device_math", "guide_rescue_host.cpp")], check=True)
    lib = C.CDLL(so)
    lib.gr_host_select.restype = C.c_int
    return lib


def host_select(lib, T, N, read, status, low, high, min_margin, max_T):
    T, N, read, low, high = (np.ascontiguousarray(v, dtype=np.uint32) for v in (T, N, read, low, high))
    status = np.ascontiguousarray(status, dtype=np.int32)
    code = np.zeros(len(status), dtype=np.uint8)
    lst = np.full(max(1, len(T)), NONE, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n = lib.gr_host_select(C.c_int(len(T)), p(T), p(N), p(read), p(status), p(low), p(high), C.c_uint32(int(min_margin)),
                           C.c_uint32(int(max_T)), p(code), p(lst))
    return code, lst[:n].tolist()


# ---- arenas -----------------------------------------------------------------------------------------------------------------
def band_arena_bytes(T, hw):
    """band_reads.hip's formula for the align job with probabilities: 25 B per band slot, rounded up to 256"""
    return (int(T) * (2 * int(hw) + 3) * 25 + 255) & ~255


def t_fit(Ts, hw, room):
    """the longest T of ``Ts`` whose arena fits ``room`` bytes (0: none)"""
    fits = [int(t) for t in Ts if band_arena_bytes(t, hw) <= room]
    return max(fits) if fits else 0


def fetch_rescue(L, handle, aligner, n):
    """dyn_batch_fetch_rescue on a raw handle: (code, rounds, converged); raises what the Python binding raises"""
    from dynamont_amd import _native as N
    from dynamont_amd._dynamont import _raise
    code, rounds, conv = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    r = L.dyn_batch_fetch_rescue(handle, code.ctypes.data_as(N.c_u8_p), rounds.ctypes.data_as(N.c_u32_p), conv.ctypes.data_as(N.c_u32_p), n)
    if r != N.DYN_OK:
        _raise(r, aligner.last_error())
    return code, rounds, conv


# ---- the reads of the GPU tests ---------------------------------------------------------------------------------------------
def mixed(fam):
    """24 of a and the 16 stall reads interleaved, eight blocks of (a, stall, a, stall, a): (reads, index of every stall read,
    of every a read)"""
    reads, stall_at, a_at = [], [], []
    a, s = list(fam["a"]), list(fam["stall"])
    for _ in range(8):
        for src, at in ((a, a_at), (s, stall_at), (a, a_at), (s, stall_at), (a, a_at)):
            at.append(len(reads))
            reads.append(src.pop(0))
    assert not a and not s
    return reads, stall_at, a_at
