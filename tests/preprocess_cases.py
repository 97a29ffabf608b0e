"""Inputs and NumPy references for tests/test_gpu_preprocess_kernels.py (launch_preprocess through tests/device_math/
preprocess.hip). Everything here runs on the CPU: the batches, the restatement of the reference workers' preprocessing
(`_numpy_prep` of tests/test_gpu_preprocess.py, whose `hampel` tests/test_harness.py pins to the reference's outputs) and
the deliberately different restatements the guards compare it with.

An instantiation is (f32, code): f32 = the arithmetic type REAL is float (train.py) or double (segment.py); code = the
library's raw_dtype, 0 float32 picoampere, 1 int16 ADC counts, 2 float64, 3 int16 ADC counts with a per-read calibration."""
import functools

import numpy as np

from test_gpu_preprocess import _numpy_prep

COMBOS = [(f32, code) for f32 in (False, True) for code in (0, 1, 2, 3)]
COMBO_IDS = ["%s-%s" % ("float" if f32 else "double", ("f32", "i16", "f64", "i16cal")[code]) for f32, code in COMBOS]
WINDOWS = list(range(1, 17))
N_SIGMAS = [0.0, 3.0, 5.0, 1e9]
ADC_PER_PA = 5.7          # the uncalibrated int16 reads: counts = rint(pA * 5.7), shift and scale in counts
POISON = 0xA5
POISON_F64 = np.frombuffer(bytes([POISON]) * 8, dtype=np.float64)[0]
GUARD = 64                # output slots behind the last read: must keep the poison
MAX_GRID_Y = 65535        # segment_kernels.hpp: reads per launch slice
TRIP = 1024 * 256         # preprocess_t: samples one trip of the grid-stride loop covers (1024 blocks of 256 threads)


class Batch:
    """raw [total] of the instantiation's sample type, offs [n + 1], shift / scale [n] float64, cal = (offset, scale) [n]
    float32 or None; reads = the per-read views of raw"""

    def __init__(self, code, reads, shift, scale, cal):
        self.code = code
        self.n = len(reads)
        self.offs = np.zeros(self.n + 1, dtype=np.uint64)
        np.cumsum([len(r) for r in reads], out=self.offs[1:])
        dt = {0: np.float32, 1: np.int16, 2: np.float64, 3: np.int16}[code]
        self.raw = np.concatenate(reads).astype(dt, copy=False) if self.n else np.zeros(0, dtype=dt)
        assert all(r.dtype == dt for r in reads)
        self.shift = np.ascontiguousarray(shift, dtype=np.float64)
        self.scale = np.ascontiguousarray(scale, dtype=np.float64)
        self.cal = None if cal is None else (np.ascontiguousarray(cal[0], dtype=np.float32), np.ascontiguousarray(cal[1], dtype=np.float32))
        assert (self.cal is not None) == (code == 3)
        for a in (self.raw, self.offs, self.shift, self.scale) + (self.cal or ()):
            a.setflags(write=False)

    def read(self, i):
        return self.raw[int(self.offs[i]):int(self.offs[i + 1])]

    def total(self):
        return int(self.offs[-1])


def picoampere(adc, off, sc, in_f64=False):
    """what pod5's signal_pa hands the reference's worker: float32 arithmetic, one operation each. in_f64: the same formula
    in float64 (NOT the reference's value: the guards use it to show that the inputs can tell the two apart)"""
    if in_f64:
        return (adc.astype(np.float64) + np.float64(off)) * np.float64(sc)
    return (adc.astype(np.float32) + np.float32(off)) * np.float32(sc)


def restate(b, W, ns, f32, reads=None, pa_in_f64=False, shift=None, scale=None, cal=None):
    """the NumPy restatement of reads `reads` (default: all) of batch b, concatenated. shift and scale go in as Python
    floats: a np.float64 scalar would promote the in-place float32 arithmetic under NumPy 2."""
    shift = b.shift if shift is None else shift
    scale = b.scale if scale is None else scale
    cal = b.cal if cal is None else cal
    out = []
    for i in (range(b.n) if reads is None else reads):
        x = b.read(i)
        if b.code == 3:
            x = picoampere(x, cal[0][i], cal[1][i], pa_in_f64)
        out.append(_numpy_prep(x, float(shift[i]), float(scale[i]), W, float(ns), f32))
    return np.concatenate(out) if out else np.zeros(0)


# ---- (a) every instantiation x every window ------------------------------------------------------------------------------
def lengths(W):
    return [0, 1, W - 1, W, W + 1, W + 2, W + 3, 57, 1000]


def _spikes(rng, pa, lo, hi, every=20):
    """spikes of both signs on pa[lo:hi]"""
    n = max(2, (hi - lo) // every)
    at = rng.integers(lo, hi, size=n)
    pa[at] += np.where(np.arange(n) % 2 == 0, 1.0, -1.0) * rng.choice([55.0, 70.0, 200.0], size=n)


def picoampere_read(rng, size, W):
    """one read in picoampere (float64). Reads of 57 and 1000 samples carry, besides Gaussian samples with spikes of both
    signs: a flat run longer than W (MAD 0, nothing to replace), a flat run with one spike inside it (MAD 0, the spike is
    replaced whatever n_sigmas is); the read of 1000 also runs of exact duplicates around the median and a two-level stretch
    whose levels change every W // 2 samples, so that an even window holds as many of one level as of the other and its
    median is the mean of two different values."""
    pa = rng.normal(90.0, 15.0, size)
    if size >= 4:
        _spikes(rng, pa, 0, size)
    if size >= 57:
        pa[3:3 + W + 2] = pa[3]                               # flat, longer than W
        pa[25:25 + W + 1] = pa[25]                            # flat with a spike at a window's centre
        pa[25 + W // 2] += 40.0 if W & 1 else -40.0
    if size >= 1000:
        pa[100:100 + 2 * W + 8] = pa[100]                     # the same two at a length where several windows are flat
        pa[150:150 + 2 * W + 5] = pa[150]
        pa[150 + W + 2] -= 35.0
        pa[200:300] = 90.0 + 0.5 * rng.choice([-1.0, 0.0, 0.0, 0.0, 1.0], size=100)     # exact duplicates around the median
        k = max(1, W // 2)
        pa[300:400] = np.where((np.arange(100) // k) % 2 == 0, 82.25, 97.5)             # two levels
        pa[400:420] = np.where(np.arange(20) % 2 == 0, 82.25, 97.5)                     # ... alternating sample by sample
    return pa


@functools.lru_cache(maxsize=None)
def window_batch(f32, code, W):
    """the batch of one (instantiation, W): every read its own shift, scale and calibration; the int16 reads of 57 and 1000
    samples hold -32768 and 32767"""
    rng = np.random.default_rng(1000 * W + 10 * code + int(f32))
    reads, shift, scale, co, cs = [], [], [], [], []
    for size in lengths(W):
        pa = picoampere_read(rng, size, W)
        sh, sc = rng.uniform(80.0, 100.0), rng.uniform(10.0, 20.0)
        off, csc = np.float32(rng.uniform(-260.0, -200.0)), np.float32(rng.uniform(0.15, 0.2))
        if code == 0:
            raw = pa.astype(np.float32)
        elif code == 2:
            raw = pa
        else:
            raw = np.rint(pa * ADC_PER_PA if code == 1 else pa / float(csc) - float(off)).astype(np.int16)
            if code == 1:
                sh, sc = sh * ADC_PER_PA, sc * ADC_PER_PA
            if size >= 57:
                raw[50], raw[54] = -32768, 32767              # (behind the flat runs of every W)
        reads.append(raw)
        shift.append(sh)
        scale.append(sc)
        co.append(off)
        cs.append(csc)
    return Batch(code, reads, shift, scale, (co, cs) if code == 3 else None)


@functools.lru_cache(maxsize=None)
def window_want(f32, code, W, ns):
    w = restate(window_batch(f32, code, W), W, ns, f32)
    w.setflags(write=False)
    return w


# ---- samples exactly on the threshold --------------------------------------------------------------------------------------
# The Gaussian batches never put a sample ON the threshold, so `>=` in place of `>`, the constant 1.4826 rounded to float32
# in the float64 kernel, or n_sigmas * sigma formed in float64 in the float32 kernel all pass them. Here shift = 0 and
# scale = 1 (the raw values ARE the normalised ones), W = 3 and every read is (-m, x, 0, 0, 0): the window of centre 1
# sorts to (-m, 0, x), its median is 0, its deviations are (m, x, 0), MAD = m, so the centre is replaced (by 0) exactly
# when x > thr = REAL(n_sigmas) * (REAL(1.4826) * m). Three reads per m: x = thr (kept), the next value above (replaced),
# the next below (kept).
THRESHOLD_COMBOS = [(False, 2), (True, 0), (True, 2)]      # raw types that carry a REAL value exactly
THRESHOLD_IDS = ["double-f64", "float-f32", "float-f64"]
THRESHOLD_NS = [3.0, 5.0]
THRESHOLD_M = 24


def threshold_values(f32, ns):
    """(m [THRESHOLD_M], thr [THRESHOLD_M]) in the arithmetic type"""
    t = np.float32 if f32 else np.float64
    m = np.random.default_rng(5).uniform(0.5, 2.0, THRESHOLD_M).astype(t)
    return m, t(ns) * (t(1.4826) * m)


@functools.lru_cache(maxsize=None)
def threshold_batch(f32, code, ns):
    t = np.float32 if f32 else np.float64
    dt = np.float32 if code == 0 else np.float64
    m, thr = threshold_values(f32, ns)
    reads = []
    for mk, tk in zip(m, thr):
        for x in (tk, np.nextafter(tk, t(np.inf)), np.nextafter(tk, t(0))):
            reads.append(np.array([-mk, x, 0, 0, 0], dtype=t).astype(dt))
    return Batch(code, reads, [0.0] * len(reads), [1.0] * len(reads), None)


# ---- (b) the grid-stride trips -------------------------------------------------------------------------------------------
TRIP_LENGTHS = [TRIP - 1, 0, TRIP, 5, TRIP + 1, 1000, 600001]
TRIP_SPIKES = list(range(TRIP - 3, TRIP + 4)) + list(range(2 * TRIP - 2, 2 * TRIP + 3))   # 262 141..262 147, 524 286..524 290
TRIP_SETTINGS = {"double-i16cal-W3": (False, 3, 3, 3.0), "float-f32-W7": (True, 0, 7, 5.0)}    # f32, code, W, n_sigmas


@functools.lru_cache(maxsize=None)
def trip_batch(code):
    rng = np.random.default_rng(77 + code)
    reads, shift, scale, co, cs = [], [], [], [], []
    for size in TRIP_LENGTHS:
        pa = rng.normal(90.0, 15.0, size)
        if size >= 1000:
            _spikes(rng, pa, 0, size, every=50)
        for k, at in enumerate(TRIP_SPIKES):   # every second one an outlier among its neighbours (a run of equal spikes is a plateau
            if at < size:                      # no window rejects): 262 142, 262 144, 262 146, 524 286, 524 288, 524 290
                pa[at] = 90.0 + (200.0 + k) * (1.0 if k % 4 == 1 else -1.0) if k % 2 else 110.0 + k
        off, csc = np.float32(rng.uniform(-260.0, -200.0)), np.float32(rng.uniform(0.15, 0.2))
        reads.append(pa.astype(np.float32) if code == 0 else np.rint(pa / float(csc) - float(off)).astype(np.int16))
        shift.append(rng.uniform(80.0, 100.0))
        scale.append(rng.uniform(10.0, 20.0))
        co.append(off)
        cs.append(csc)
    return Batch(code, reads, shift, scale, (co, cs) if code == 3 else None)


@functools.lru_cache(maxsize=None)
def trip_want(name):
    f32, code, W, ns = TRIP_SETTINGS[name]
    w = restate(trip_batch(code), W, ns, f32)
    w.setflags(write=False)
    return w


# ---- (c) more reads than one launch slice --------------------------------------------------------------------------------
MANY_READS = MAX_GRID_Y + 6
MANY_SETTINGS = {"double-i16cal": (False, 3), "float-f32": (True, 0)}
MANY_W, MANY_NS = 3, 3.0


@functools.lru_cache(maxsize=None)
def many_batch(code):
    """65 541 reads of 0 .. 9 samples (read r has r % 10), every per-read value distinct"""
    rng = np.random.default_rng(4242 + code)
    r = np.arange(MANY_READS)
    lens = r % 10
    pa = rng.normal(90.0, 15.0, int(lens.sum()))
    pa[rng.integers(0, len(pa), size=len(pa) // 6)] += 80.0
    shift = 80.0 + r * (20.0 / MANY_READS)
    scale = 10.0 + r * (10.0 / MANY_READS)
    co = (-260.0 + r * 2.0 ** -11).astype(np.float32)          # exact in float32: 65 541 distinct values
    cs = (0.15 + r * 2.0 ** -21).astype(np.float32)
    assert len(np.unique(co)) == MANY_READS and len(np.unique(cs)) == MANY_READS
    ends = np.cumsum(lens)
    if code == 0:
        raw = pa.astype(np.float32)
    else:
        raw = np.rint(pa / np.repeat(cs.astype(np.float64), lens) - np.repeat(co.astype(np.float64), lens)).astype(np.int16)
    reads = [raw[e - n:e] for e, n in zip(ends.tolist(), lens.tolist())]
    return Batch(code, reads, shift, scale, (co, cs) if code == 3 else None)


@functools.lru_cache(maxsize=None)
def many_want(name):
    f32, code = MANY_SETTINGS[name]
    w = restate(many_batch(code), MANY_W, MANY_NS, f32)
    w.setflags(write=False)
    return w
