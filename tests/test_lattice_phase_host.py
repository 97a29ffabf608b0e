"""CPU: the one decode of the lattice phases (dynamont_amd/csrc/lattice_phase.hpp) compiled with g++ behind an extern "C" shim,
against a restatement in Python of the two ladders it replaced: the one launch_read_queue walked (nt_kernels.hip) and the one
launch_band_reads walked with expressions of its own (band_reads.hip). Both launches now take the phases of a launch from the
header, so what is pinned here is pinned for both kernels."""
import ctypes as C
import itertools
import subprocess

import pytest

from conftest import ROOT

SRC = r'''
#include "%s/dynamont_amd/csrc/lattice_phase.hpp"
extern "C" {
int lp_phases(int align_calc, int tag_word, double tail, int border_window) { return dynk::lattice_phases(align_calc != 0, tag_word, tail, border_window); }
int lp_bit(int i) { const int b[] = {dynk::JOB_BORDER, dynk::JOB_SAMPLE, dynk::JOB_INTERVAL, dynk::JOB_SOFT, dynk::LATTICE_PHASE_BITS}; return b[i]; }
int lp_soft_tag() { return dynk::SOFT_TAG; }
int lp_n_sets() { return dynk::N_LATTICE_PHASE_SETS; }
int lp_set(int i) { return dynk::LATTICE_PHASE_SETS[i]; }
}
''' % ROOT

BORDER, SAMPLE, INTERVAL, SOFT = 8, 16, 32, 64
SOFT_TAG = -1
LEGAL = [0, BORDER, SAMPLE, SAMPLE | BORDER, INTERVAL, SOFT]

TAG_WORDS = (SOFT_TAG, -2, 0, 1, 64)
TAILS = (0.0, 0.05)
WINDOWS = (0, 1, 256)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("latticephase")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    L.lp_phases.restype = C.c_int
    L.lp_phases.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int]
    return L


def read_queue_ladder(align_calc, tag_word, tail, border_window):
    """launch_read_queue as it was: four blocks in this order, each behind `job == JOB_ALIGN || job == JOB_ALIGN_INPLACE`, the
    first that holds launches; behind them the launches without a phase"""
    if tag_word == SOFT_TAG and align_calc:                    # q.soft.tag == SOFT_TAG
        return SOFT
    if tag_word == 0 and tail > 0.0 and align_calc:            # q.sample.count == 0 && q.interval.tail > 0.0
        return INTERVAL
    if tag_word > 0 and align_calc:                            # q.sample.count > 0
        return SAMPLE | (BORDER if border_window > 0 else 0)   # ... behind the border-confidence phase
    if border_window > 0 and align_calc:                       # q.border_window > 0
        return BORDER
    return 0


def band_reads_ladder(job, tag_word, tail, border_window):
    """launch_band_reads' diagonal branch as it was, behind its refusals: `soft` and `interval` formed up front, then the kernels
    in the order sample(border) / interval / soft / border / plain. The refusals stand between: the soft levels and the
    intervals beside a border window, a negative count other than SOFT_TAG. None: refused."""
    soft = job == 1 and tag_word == SOFT_TAG
    if soft and border_window > 0:
        return None
    if not soft and job == 1 and tag_word < 0:
        return None
    interval = job == 1 and tag_word == 0 and tail > 0.0
    if interval and border_window > 0:
        return None
    if border_window > 0 and job != 1:
        return None
    if job == 1 and tag_word > 0:
        return SAMPLE | (BORDER if border_window > 0 else 0)
    if interval:
        return INTERVAL
    if soft:
        return SOFT
    if border_window > 0:
        return BORDER
    return 0


def test_constants_and_the_list_of_sets(lib):
    assert [lib.lp_bit(i) for i in range(5)] == [BORDER, SAMPLE, INTERVAL, SOFT, BORDER | SAMPLE | INTERVAL | SOFT]
    assert lib.lp_soft_tag() == SOFT_TAG
    assert [lib.lp_set(i) for i in range(lib.lp_n_sets())] == LEGAL


def test_the_decode_is_both_ladders(lib):
    seen = set()
    for align_calc, tag_word, tail, window in itertools.product((True, False), TAG_WORDS, TAILS, WINDOWS):
        got = lib.lp_phases(int(align_calc), tag_word, tail, window)
        case = (align_calc, tag_word, tail, window)
        assert got in LEGAL, case
        assert got == read_queue_ladder(align_calc, tag_word, tail, window), case
        # the banded-lattice launch: job 1 is align with probabilities, jobs 0 and 2 (Z only, train) never carry a phase
        for job in ((1,) if align_calc else (0, 2)):
            want = band_reads_ladder(job, tag_word, tail, window)
            if want is not None:                               # (what it refuses it refuses before it asks)
                assert got == want, (job,) + case
        seen.add(got)
    assert seen == set(LEGAL)                                  # the cases reach every set the launches instantiate
    assert not any(lib.lp_phases(0, t, tl, w) for t, tl, w in itertools.product(TAG_WORDS, TAILS, WINDOWS))
