"""The preprocessing kernels (preprocess_kernels.hpp: k_normalise, k_hampel, launch_preprocess) pinned sample for sample.

tests/device_math/preprocess.hip, compiled with the product's flags, hands the product's own launch arrays built on the host
(tests/preprocess_cases.py); every output sample is compared with the NumPy restatement of the reference workers'
preprocessing (`_numpy_prep`, tests/test_gpu_preprocess.py) with np.array_equal -- no tolerance anywhere.

  a. all eight (REAL, RAW, calibration) instantiations x W = 1 .. 16 x n_sigmas in {0, 3, 5, 1e9}
     and samples placed exactly on, one value above and one value below the threshold n_sigmas * 1.4826 * MAD
  b. reads of up to three trips of the grid-stride loop, spikes across the trip boundaries
  c. 65 541 reads: the second launch slice, every per-read array distinct in every read
  d. launches with nothing to do

Not GPU-marked: that the harness compiles, and the guards -- the inputs can tell a filter that did nothing, float64
arithmetic in place of float32, picoampere formed in float64 and a slice without its read offset from the right result.

What the filter can do at W = 1 and W = 2 (the guard "n_sigmas 3.0 differs from 1e9" cannot hold there for any input): a
window of one sample is its own median, |x - med| = 0 is never > anything, the filter is the identity for every n_sigmas.
In a window of two, med = (a + b) / 2 and both deviations are |a - b| / 2 up to one rounding, so |x - med| <= 1.0000002 MAD
< 3 * 1.4826 MAD: nothing is replaced at 3.0, 5.0 or 1e9, and every centre whose neighbour differs is replaced at 0.0. The
guards for these two widths assert exactly that (W = 1: all four outputs equal the normalised signal; W = 2: 0.0 differs
from 1e9); from W = 3 on, 3.0 must differ from 1e9.

No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import preprocess_cases as pc
from conftest import ROOT
from dynamont_amd import _native

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def harness_so(tmp_path_factory):
    """tests/device_math/preprocess.hip -> a shared library, with the flags of every translation unit of the product"""
    so = tmp_path_factory.mktemp("preprocess") / "libpreprocess.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/preprocess.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(so)


@pytest.fixture(scope="module")
def lib(harness_so):
    L = C.CDLL(harness_so)
    L.pp_run.restype = C.c_int
    return L


def run_on_device(lib, b, W, ns, f32):
    """pp_run -> the float64 output of every read, concatenated; every HIP call must have returned hipSuccess and the
    GUARD slots behind the last read must still hold the poison"""
    n_out = b.total() + pc.GUARD
    out = np.zeros(n_out)
    err = np.full(32, -1, dtype=np.int32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    co, cs = b.cal if b.cal is not None else (None, None)
    k = lib.pp_run(p(b.raw), C.c_int(b.code), C.c_int(int(f32)), C.c_int(b.n), p(b.offs), p(b.shift), p(b.scale), p(co), p(cs),
                   C.c_int(W), C.c_double(ns), C.c_int(pc.POISON), C.c_uint64(n_out), p(out), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert (out[b.total():].view(np.uint64) == np.float64(pc.POISON_F64).view(np.uint64)).all()
    return out[:b.total()]


def first_difference(b, got, want):
    """text for the first samples that differ, or None"""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    bad = np.flatnonzero(got != want)[:5]
    reads = np.searchsorted(b.offs, bad, side="right") - 1
    return "; ".join("read %d (%d samples) sample %d: device %r, NumPy %r" % (r, int(b.offs[r + 1] - b.offs[r]), i - int(b.offs[r]), got[i], want[i])
                     for i, r in zip(bad.tolist(), reads.tolist()))


# ---- not GPU-marked ----------------------------------------------------------------------------------------------------------
def test_harness_compiles_with_the_products_flags(harness_so):
    assert os.path.getsize(harness_so) > 0


@pytest.mark.parametrize("f32,code", pc.COMBOS, ids=pc.COMBO_IDS)
def test_window_batches_can_fail(f32, code):
    """The guards of (a), for every W, on the restatement alone."""
    for W in pc.WINDOWS:
        b = pc.window_batch(f32, code, W)
        assert [len(b.read(i)) for i in range(b.n)] == pc.lengths(W)
        for a in (b.shift, b.scale) + (b.cal or ()):
            assert len(np.unique(a)) == b.n                                             # every read its own values
        if code in (1, 3):
            assert b.raw.min() == -32768 and b.raw.max() == 32767
        want = {ns: pc.window_want(f32, code, W, ns) for ns in pc.N_SIGMAS}
        assert all(np.isfinite(w).all() for w in want.values())
        if W == 1:      # a window of one sample: the identity (module docstring)
            assert all(np.array_equal(want[ns], want[0.0]) for ns in pc.N_SIGMAS)
        elif W == 2:    # two samples: nothing exceeds 3 sigma, everything exceeds 0
            assert np.array_equal(want[3.0], want[1e9]) and np.any(want[0.0] != want[1e9])
        else:
            assert np.any(want[3.0] != want[1e9]), W                                   # the filter did something
            assert np.any(want[0.0] != want[3.0]) and np.any(want[3.0] != want[5.0]), W
        # the flat run with a spike inside it (read of 57 samples): replaced whatever n_sigmas is, from W = 3 on
        if W >= 3:
            r57 = slice(int(b.offs[7]), int(b.offs[8]))
            at = 25 + W // 2
            w = want[1e9][r57]
            assert w[at] == w[25] and w[at - 1] == w[25], W
        if f32:         # float64 arithmetic gives another sample somewhere
            assert np.any(pc.restate(b, W, 3.0, False) != want[3.0]), W
        if code == 3:   # ... and so does picoampere formed in float64
            assert np.any(pc.restate(b, W, 3.0, f32, pa_in_f64=True) != want[3.0]), W
        if not W & 1 and W > 2:   # the two-level stretch: a window median that is the mean of two different values
            r1000 = slice(int(b.offs[8]), int(b.offs[9]))
            t = np.float32 if f32 else np.float64
            levels = np.unique(want[1e9][r1000][300:400])
            assert len(levels) == 2, W
            assert np.any(want[0.0][r1000][300:400] == np.float64((t(levels[0]) + t(levels[1])) / t(2))), W


@pytest.mark.parametrize("f32,code", pc.THRESHOLD_COMBOS, ids=pc.THRESHOLD_IDS)
def test_threshold_batch_can_fail(f32, code):
    """x == threshold is kept, the next value above it is replaced, and the three near misses of the comparison --
    `>=`, the float32 constant in the float64 kernel, the float64 product in the float32 kernel -- would decide otherwise."""
    t = np.float32 if f32 else np.float64
    for ns in pc.THRESHOLD_NS:
        b = pc.threshold_batch(f32, code, ns)
        m, thr = pc.threshold_values(f32, ns)
        want = pc.restate(b, 3, ns, f32).reshape(pc.THRESHOLD_M, 3, 5)
        assert np.array_equal(want[:, :, 0], np.repeat(-m.astype(np.float64), 3).reshape(-1, 3)) and not want[:, :, 2:].any()
        assert np.array_equal(want[:, 0, 1], thr.astype(np.float64))          # on the threshold: kept (`>=` would give 0)
        assert not want[:, 1, 1].any()                                        # one value above: replaced by the median, 0
        assert np.array_equal(want[:, 2, 1], np.nextafter(thr, t(0)).astype(np.float64))
        if f32:   # n_sigmas * sigma in float64: below the float32 product for some m (x == thr would be replaced)
            exact = ns * (np.float32(1.4826) * m).astype(np.float64)
            assert (exact < thr).any() and (exact > thr).any()
        else:     # 1.4826f: a threshold more than one value away, on the side that flips x == thr or the value above it
            other = ns * (np.float64(np.float32(1.4826)) * m)
            assert ((other < thr) | (other > np.nextafter(thr, np.inf))).all()


@pytest.mark.parametrize("name", list(pc.TRIP_SETTINGS))
def test_trip_batch_can_fail(name):
    f32, code, W, ns = pc.TRIP_SETTINGS[name]
    b = pc.trip_batch(code)
    assert sorted(len(b.read(i)) for i in range(b.n)) == [0, 5, 1000, 262143, 262144, 262145, 600001]
    want, plain = pc.trip_want(name), pc.restate(b, W, 1e9, f32)
    assert pc.TRIP_SPIKES == list(range(262141, 262148)) + list(range(524286, 524291))
    for i in range(b.n):      # the filter replaces samples on both sides of every trip boundary a read reaches well past
        o, n = int(b.offs[i]), len(b.read(i))
        changed = np.flatnonzero(want[o:o + n] != plain[o:o + n])
        for edge in (pc.TRIP, 2 * pc.TRIP):
            if n >= edge + 8:
                assert ((changed >= edge - 4) & (changed < edge)).any() and ((changed >= edge) & (changed < edge + 4)).any(), (i, edge)
                assert edge in changed, (i, edge)     # the first sample of a trip, its window reaching back into the one before


@pytest.mark.parametrize("name", list(pc.MANY_SETTINGS))
def test_many_reads_batch_can_fail(name):
    """A slice that takes one of the five per-read arrays without its read offset gives another sample: the reads of the
    second slice, restated with the values of the reads MAX_GRID_Y in front of them, differ from the right result."""
    f32, code = pc.MANY_SETTINGS[name]
    b = pc.many_batch(code)
    assert b.n == 65541 and b.n > pc.MAX_GRID_Y and b.total() < 300_000
    assert [len(b.read(i)) for i in range(20)] == list(range(10)) * 2
    tail = list(range(pc.MAX_GRID_Y, b.n))
    right = pc.restate(b, pc.MANY_W, pc.MANY_NS, f32, reads=tail)
    assert np.array_equal(right, pc.many_want(name)[int(b.offs[pc.MAX_GRID_Y]):]) and len(right) >= 30
    shifted = lambda a: np.concatenate([a[:pc.MAX_GRID_Y], a[:b.n - pc.MAX_GRID_Y]])  # noqa: E731  a[r - MAX_GRID_Y] for r in the tail
    assert np.any(pc.restate(b, pc.MANY_W, pc.MANY_NS, f32, reads=tail, shift=shifted(b.shift)) != right)
    assert np.any(pc.restate(b, pc.MANY_W, pc.MANY_NS, f32, reads=tail, scale=shifted(b.scale)) != right)
    if code == 3:
        assert np.any(pc.restate(b, pc.MANY_W, pc.MANY_NS, f32, reads=tail, cal=(shifted(b.cal[0]), b.cal[1])) != right)
        assert np.any(pc.restate(b, pc.MANY_W, pc.MANY_NS, f32, reads=tail, cal=(b.cal[0], shifted(b.cal[1]))) != right)
    head = range(2000)
    assert np.any(pc.many_want(name)[:int(b.offs[2000])] != pc.restate(b, pc.MANY_W, 1e9, f32, reads=head))   # the filter did something
    assert not np.array_equal(b.offs[pc.MAX_GRID_Y:pc.MAX_GRID_Y + 7], b.offs[:7])     # (offsets: a read of the wrong place)


# ---- on the device -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("W", pc.WINDOWS)
@pytest.mark.parametrize("f32,code", pc.COMBOS, ids=pc.COMBO_IDS)
def test_every_instantiation_every_window(lib, f32, code, W):
    b = pc.window_batch(f32, code, W)
    for ns in pc.N_SIGMAS:
        bad = first_difference(b, run_on_device(lib, b, W, ns, f32), pc.window_want(f32, code, W, ns))
        assert bad is None, "W %d, n_sigmas %g: %s" % (W, ns, bad)


@gpu
@pytest.mark.parametrize("f32,code", pc.THRESHOLD_COMBOS, ids=pc.THRESHOLD_IDS)
def test_samples_on_the_threshold(lib, f32, code):
    for ns in pc.THRESHOLD_NS:
        b = pc.threshold_batch(f32, code, ns)
        bad = first_difference(b, run_on_device(lib, b, 3, ns, f32), pc.restate(b, 3, ns, f32))
        assert bad is None, "n_sigmas %g: %s" % (ns, bad)


@gpu
@pytest.mark.parametrize("name", list(pc.TRIP_SETTINGS))
def test_grid_stride_trips(lib, name):
    f32, code, W, ns = pc.TRIP_SETTINGS[name]
    b = pc.trip_batch(code)
    bad = first_difference(b, run_on_device(lib, b, W, ns, f32), pc.trip_want(name))
    assert bad is None, bad


@gpu
@pytest.mark.parametrize("name", list(pc.MANY_SETTINGS))
def test_more_reads_than_one_launch_slice(lib, name):
    f32, code = pc.MANY_SETTINGS[name]
    b = pc.many_batch(code)
    bad = first_difference(b, run_on_device(lib, b, pc.MANY_W, pc.MANY_NS, f32), pc.many_want(name))
    assert bad is None, bad


@gpu
@pytest.mark.parametrize("f32,code", [(False, 3), (True, 0), (False, 1), (True, 2)], ids=["double-i16cal", "float-f32", "double-i16", "float-f64"])
def test_degenerate_launches(lib, f32, code):
    dt = {0: np.float32, 1: np.int16, 2: np.float64, 3: np.int16}[code]
    cal = ([-230.5] * 5, [0.17] * 5) if code == 3 else None
    empty = pc.Batch(code, [np.zeros(0, dtype=dt)] * 5, [90.0] * 5, [15.0] * 5, cal)             # max_len == 0
    assert run_on_device(lib, empty, 3, 3.0, f32).size == 0
    one = pc.Batch(code, [np.array([517], dtype=dt)], [90.25], [15.5], None if cal is None else ([-230.5], [0.17]))
    got = run_on_device(lib, one, 3, 3.0, f32)
    assert first_difference(one, got, pc.restate(one, 3, 3.0, f32)) is None and got.size == 1
    none = pc.Batch(code, [], [], [], ([], []) if code == 3 else None)                          # n_reads == 0: no launch
    assert run_on_device(lib, none, 3, 3.0, f32).size == 0
