"""CPU: the host half of the per-read signal rescaling (ABI 10). The library reports ABI 10 and exports the new entry
points; the switch is range-checked with a message on a host-only handle; the NumPy restatement of the definition
(tests/rescale_chain.py) recovers exact affine maps and applies its guards; driven pass by pass through the CPU oracle it
recovers the distortion of synthetic rna004 and dna_r10_400bps reads and moves their borders back towards those of the
undistorted reads -- the run that fixed the thresholds of tests/test_gpu_rescale.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from dynamont_amd import Aligner, synth
from dynamont_amd import _native as N
from dynamont_amd.segmentation import segment as seg
from oracle.pyoracle import Oracle
from rescale_chain import (DISTORTIONS, RECOVERY_AGREEMENT, RECOVERY_ITERS, RECOVERY_PARAM_TOL, border_agreement, fit,
                           rescale_chain, segment_means)

pytestmark = pytest.mark.usefixtures("native_lib")


def test_abi_10_and_the_new_symbols(native_lib, models):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION 10\b", hdr)
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_rescale", "dyn_batch_fetch_rescale"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "typedef struct dyn_rescale_out" in hdr and "DYN_RESCALE_MAX_ITERS 8" in hdr
    al = Aligner(models["syn9"], "rna004", device="host")
    info = N.DynInfo()
    assert native_lib.dyn_aligner_info(al._h, C.byref(info)) == 0 and info.abi_version == 10
    al.close()


def test_switch_range_on_a_host_handle(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    for bad in (-1, 9, 100):
        with pytest.raises(ValueError, match="iters must be 0 .. 8"):
            al.set_rescale(bad)
    assert al._rescale == 0
    for ok in (0, 1, 8, 0):
        al.set_rescale(ok)
        assert al._rescale == ok
    assert N.lib().dyn_aligner_set_rescale(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    al.close()


def test_cli_flag():
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    assert seg.parse(base).rescale_iters == 0
    assert seg.parse(base + ["--rescale-iters", "8"]).rescale_iters == 8
    for bad in ("9", "-1"):
        with pytest.raises(SystemExit):
            seg.parse(base + ["--rescale-iters", bad])


def test_restatement_recovers_an_exact_affine_map():
    rng = np.random.default_rng(1)
    for n in (16, 32, 64, 128, 256, 512):                   # one and several chunks of 64 rows
        m = rng.integers(-32, 33, n) / 8.0                  # dyadic, n a power of two: every step below is exact
        for b_true, a_true in ((1.25, 0.5), (0.5, -2.0), (2.0, 2.0), (0.75, 0.0)):
            y = b_true * m + a_true
            a, b, ok = fit(m, y)
            assert ok and b == b_true and a == a_true, (n, b, a)
    m = rng.integers(-32, 33, 128) / 8.0
    assert not fit(m[:15], 1.25 * m[:15] + 0.5)[2]          # fewer than 16 rows
    assert not fit(np.full(40, 0.5), rng.normal(size=40))[2]   # Sxx = 0
    assert not fit(m, 2.5 * m)[2] and not fit(m, 0.25 * m)[2]  # b outside [0.5, 2]
    assert not fit(m, m + 2.5)[2] and not fit(m, m - 3.0)[2]   # |a| > 2
    assert fit(m, 2.0 * m)[2] and fit(m, 0.5 * m - 2.0)[2]     # the bounds themselves are in
    y = 1.25 * m + 0.5
    y[3] = np.nan
    assert not fit(m, y)[2]


def test_chain_composes_the_transforms():
    """an aligner stand-in with fixed borders: x0 = 1.25 level + 0.5 per segment; the first fit finds (1.25, 0.5), the
    second the identity, so (A, B) stays (0.5, 1.25) and x_1 = x_2 are the model levels"""
    k = 9
    rng = np.random.default_rng(2)
    n = 128
    kmers = rng.integers(0, 4 ** k, n)
    mean = rng.integers(-40, 41, 4 ** k) / 16.0
    dwell = rng.integers(1, 30, n)
    sp = np.concatenate([[0], np.cumsum(dwell)[:-1]]).astype(np.uint64)
    x0 = np.repeat(1.25 * mean[kmers] + 0.5, dwell)
    seen = []

    def align(x, seq):
        seen.append(x.copy())
        return dict(signal_positions=sp, sequence_positions=np.arange(n, dtype=np.uint64) + k // 2)

    ch = rescale_chain(align, x0, "", mean, kmers, k, 2)
    assert [p["iters_applied"] for p in ch] == [0, 1, 2]
    assert (ch[1]["shift"], ch[1]["scale"]) == (0.5, 1.25) and (ch[2]["shift"], ch[2]["scale"]) == (0.5, 1.25)
    assert np.array_equal(seen[0], x0) and np.array_equal(seen[1], mean[kmers].repeat(dwell))
    assert np.array_equal(segment_means(seen[2], sp), mean[kmers])
    # a refused fit freezes the read: later passes align the same signal, no further fit
    ch = rescale_chain(align, np.repeat(3.0 * mean[kmers], dwell), "", mean, kmers, k, 3)
    assert [p["iters_applied"] for p in ch] == [0, 0, 0, 0] and all(p["scale"] == 1.0 and p["shift"] == 0.0 for p in ch)


def _recovery(models, pore, n_reads=16):
    model = models["syn9"]
    _, mean, sd = synth.read_model_file(model)
    orc = Oracle(model, synth.PORES[pore][0])
    mm, _ = orc.table()
    reads = synth.make_reads(7100, n_reads, pore, mean, sd, (60, 200))
    out = {}
    for bb, aa in DISTORTIONS:
        rows = []
        for r in reads:
            ref = orc.align(r.signal, r.sequence, True)
            ch = rescale_chain(lambda s, q: orc.align(s, q, True), bb * r.signal + aa, r.sequence, mm, orc.kmers(r.sequence), 9,
                               RECOVERY_ITERS)
            rows.append((border_agreement(ch[0]["res"]["signal_positions"], ref["signal_positions"]),
                         border_agreement(ch[-1]["res"]["signal_positions"], ref["signal_positions"]),
                         ch[-1]["scale"], ch[-1]["shift"], ch[-1]["iters_applied"]))
        out[(bb, aa)] = np.array(rows)
    return out


@pytest.mark.parametrize("pore", ["rna004", "dna_r10_400bps"])
def test_restatement_with_the_oracle_recovers_distortions(models, oracle_built, pore):
    for (bb, aa), rows in _recovery(models, pore).items():
        agr0, agrK, B, A, it = rows.T
        assert (it == RECOVERY_ITERS).all()
        assert np.abs(B - bb).max() <= RECOVERY_PARAM_TOL and np.abs(A - aa).max() <= RECOVERY_PARAM_TOL, (bb, aa)
        assert agrK.mean() >= RECOVERY_AGREEMENT > agr0.mean(), (bb, aa, agrK.mean(), agr0.mean())
        assert agrK.mean() > agr0.mean() + 0.2
