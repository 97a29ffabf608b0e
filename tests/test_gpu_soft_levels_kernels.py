"""GPU (-m gpu): soft_level_kernels.hpp's two sweeps, compiled into a test unit with the product's flags
(tests/device_math/soft_levels.hip), on lattices the test writes itself -- the one tests/test_gpu_border_interval.py builds (610
columns, so the band slots wrap; a band of 25; every out-of-band slot poisoned with probability 1; -inf cells inside the band) and
a second of the same kind whose band is three columns wide on a diagonal steeper than 1, where every other column has a SINGLE
in-band row. Over the three accessor pairs (separate, in place, wide) and, for the wide layout, the column walk: every sum is,
bit for bit, the host's sequential sum of the device's own terms. No stateful accessor was added: the sweeps read the lattice
through border_kernels.hpp's and sample_kernels.hpp's accessors as they are."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dynamont_amd import _native
from test_gpu_border_interval import Lattice

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("soft") / "libsoft.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/soft_levels.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.sl_run.restype = C.c_int
    return lib


@pytest.fixture(scope="module")
def lattices():
    # "steep": N / T = 1.99 and a band of 3 columns -- every column is in band for one or two rows, half of them for one
    return {"slots_wrap": Lattice(), "steep": Lattice(seed=23, T=306, N=610, bw=1, faint=301)}


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
@pytest.mark.parametrize("which", ["slots_wrap", "steep"])
def test_device_harness_sweeps(harness, lattices, which, mode):
    la = lattices[which]
    cols, W = la.N - 1, 2 * la.bw + 1
    sums = np.full((3, cols), -7.0)
    terms = np.full((la.T, W), -7.0)
    err = np.full(64, -1, dtype=np.int32)
    lp = (la.lpe_sep, la.lp_in, la.lp_wide, la.lp_wide)[mode]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = harness.sl_run(C.c_int(mode), C.c_int(la.T), C.c_int(la.N), C.c_int(la.bw), C.c_double(la.ratio), C.c_double(la.Zb),
                       C.c_double(la.m1), C.c_uint64(la.rowmap.size), p(la.rowmap), C.c_uint64(lp.size), p(lp),
                       C.c_uint64(la.bE.size), p(la.bE), C.c_uint64(la.sig.size), p(la.sig), C.c_uint64(la.par.shape[0]), p(la.par),
                       p(sums), p(terms), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    # the terms: written for exactly the in-band cells; for the layouts that store both floats, exp of exactly those floats
    for t in range(1, la.T):
        s = int(la.start[t])
        n = s + np.arange(W)
        ib = (n >= 1) & (n < la.N)
        assert (terms[t, ib] != -7.0).all() and (terms[t, ~ib] == -7.0).all(), t
        assert (terms[t, ib] >= 0.0).all() and np.isfinite(terms[t, ib]).all(), t
        if mode != 0:
            with np.errstate(over="ignore"):
                want = (np.exp(la.lp_wide[t, 1:W + 1, 0].astype(np.float64)) + np.exp(la.lp_wide[t, 1:W + 1, 1].astype(np.float64)))[ib]
            assert np.allclose(terms[t, ib], want, rtol=1e-15, atol=0.0), t
            assert (terms[t, ib] <= 1.05).all(), t                                # an E share is at most 1, an M share 0.04
    assert (terms[0] == -7.0).all()
    single = 0
    for n in range(1, la.N):
        ts = np.nonzero(la.inband[:la.T, n])[0]
        single += len(ts) == 1
        w = s1 = s2 = 0.0
        for t in ts.tolist():
            g = float(terms[t, n - int(la.start[t])])
            x = float(la.sig[t - 1])
            gx = g * x
            w = w + g
            s1 = s1 + gx
            s2 = s2 + gx * x
        got = sums[:, n - 1]
        assert np.array_equal(got.view(np.uint64), np.array([w, s1, s2]).view(np.uint64)), (which, mode, n, got.tolist(), (w, s1, s2))
    if which == "steep":
        assert single >= 100                                                      # columns with a single in-band row
    print(f"{which} mode {mode}: {cols} columns bit for bit, {single} of them with a single in-band row")
