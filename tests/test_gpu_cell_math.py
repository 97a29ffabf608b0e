"""GPU: the per-cell arithmetic (dp_math.hpp, dp_math_strict.hpp, dp_cell.hpp) as the DEVICE build computes it, function by
function, against the g++ build of the same headers -- bit pattern for bit pattern.

tests/test_dp_math.py and tests/test_dp_math_strict.py pin the HOST build of these headers to libm and mpmath. What the GPU
runs is another build of the same text: the branches behind __HIP_DEVICE_COMPILE__ (v_max_f64 / v_min_f64, the hardware ldexp,
the register pins), hipcc's division and its handling of -ffp-contract=off, and the code only the device has (dp_cell.hpp:
the wave-level fallback of the certified logPlus, the training sweep's folded emission). tests/device_math/cell_math.hip runs
each function on arrays of arguments in the sweeps' geometry (whole 64-lane waves, 7 cells per lane, 256-thread groups, tables
staged into LDS by the product's loop); the module compiles it once with the product's own flags and compares with the host
evaluation wrappers at the end of test_dp_math_strict.py's CERT_SRC. Two more builds of the same unit show that the comparison
can fail: one without the certified logPlus' fallback, one with -ffp-contract=fast.

No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import subprocess

import mpmath as mp
import numpy as np
import pytest

from conftest import ROOT
from dynamont_amd import _native
from test_dp_math import _grid7
from test_dp_math_strict import CERT_SRC, _model_stdevs

pytestmark = pytest.mark.gpu

P = 448  # cells of one wave: 64 lanes x 7 registers (nt_kernels.hpp)
(OP_EXP_STRICT, OP_LOG1P_STRICT, OP_LOG_PLUS_STRICT, OP_PDF_STRICT, OP_LOG_PLUS, OP_SOFTPLUS, OP_PDF, OP_EXP128,
 OP_EMIS_FOLDED, OP_LOG_PLUS_CERT) = range(10)  # enum Op of cell_math.hip

dp = C.POINTER(C.c_double)


class CellMath:
    """The host build (g++) and the three device builds (hipcc) of the same headers."""

    def __init__(self, d):
        src = d / "host.cpp"
        src.write_text(CERT_SRC)
        host_so = d / "libcellhost.so"
        unit = str(ROOT) + "/tests/device_math/cell_math.hip"
        flags = _native.hipcc_flags()
        assert "-ffp-contract=off" in flags
        fast = [f if f != "-ffp-contract=off" else "-ffp-contract=fast" for f in flags]
        variants = {"dev": flags, "nofb": flags + ["-DDYN_EXP_NO_CERT_FALLBACK"], "fast": fast}
        jobs = [subprocess.Popen(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(host_so), str(src)])]
        for name, fl in variants.items():
            jobs.append(subprocess.Popen([_native.hipcc_path()] + fl + ["-I", _native.CSRC, "-shared", "-x", "hip", unit,
                                                                        "-o", str(d / ("libcell_%s.so" % name))]))
        assert [j.wait() for j in jobs] == [0] * len(jobs)
        self.host = C.CDLL(str(host_so))
        for name in variants:
            L = C.CDLL(str(d / ("libcell_%s.so" % name)))
            L.cm_run.restype = C.c_int
            setattr(self, name, L)
        # the existing skip rule of test_dp_math_strict.py, as a flag: is this host's libm the glibc the strict functions restate?
        x = -np.random.default_rng(99).uniform(0, 40, 7 * 3000)
        self.libm_is_restated_glibc = int(np.sum(self.h("ev_exp_strict", [x], 1)[0] != self.h("ev_libm_exp", [x], 1)[0])) <= 20

    def h(self, fn, ins, n_out, extra=()):
        """host wrapper fn(in..., out..., [extra...], n) -> list of outputs"""
        ins = [np.ascontiguousarray(a, dtype=np.float64) for a in ins]
        n = len(ins[0])
        assert n % 7 == 0 and all(len(a) == n for a in ins)
        outs = [np.full(n, np.nan) for _ in range(n_out)]
        getattr(self.host, fn)(*[a.ctypes.data_as(dp) for a in ins + outs], *[e.ctypes.data_as(C.c_void_p) for e in extra], C.c_long(n))
        return outs

    def run(self, op, ins, n_out, lib=None, lds=True, fallbacks=False):
        """device: cm_run -> list of outputs (and the per-wave fallback counts); every HIP call must have returned hipSuccess"""
        ins = [np.ascontiguousarray(a, dtype=np.float64) for a in ins]
        n = len(ins[0])
        assert n % P == 0 and all(len(a) == n for a in ins)
        outs = [np.empty(n) for _ in range(n_out)]
        fb = np.empty(n // P, dtype=np.uint32) if fallbacks else None
        err = np.full(64, -1, dtype=np.int32)
        k = (lib or self.dev).cm_run(C.c_int(op), C.c_int(int(lds)), C.c_long(n), C.c_int(len(ins)),
                                     (C.c_void_p * len(ins))(*[a.ctypes.data for a in ins]), C.c_int(n_out),
                                     (C.c_void_p * n_out)(*[a.ctypes.data for a in outs]),
                                     C.c_void_p(fb.ctypes.data if fallbacks else None), err.ctypes.data_as(C.c_void_p))
        assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
        return outs + [fb] if fallbacks else outs


@pytest.fixture(scope="module")
def cm(tmp_path_factory):
    return CellMath(tmp_path_factory.mktemp("cellmath"))


def pad(*arrays):
    """to a multiple of 448 (every lane of every wave live), repeating the leading arguments"""
    n = len(arrays[0])
    m = -n % P
    out = [np.ascontiguousarray(np.concatenate([a, a[:m]]), dtype=np.float64) for a in arrays]
    assert all(len(a) == n + m for a in out)
    return out if len(out) > 1 else out[0]


def differing(got, want):
    return (got.view(np.uint64) != want.view(np.uint64)) & ~(np.isnan(got) & np.isnan(want))


def assert_same_bits(what, got, want, args, got_name="device", want_name="host"):
    bad = differing(got, want)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        pytest.fail("%s: %d of %d results differ; first at (%s): %s %#018x, %s %#018x" % (
            what, int(bad.sum()), len(got), ", ".join(float(a[i]).hex() for a in args),
            got_name, int(got.view(np.uint64)[i]), want_name, int(want.view(np.uint64)[i])))


def neighbours(x, k=2):
    """x and its k nearest doubles on either side"""
    x = np.asarray(x, dtype=np.float64)
    out = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


# ---- argument sets: those of the host tests (same generators and seeds) plus the edges of each function -------------------
def exp_strict_args():
    rng = np.random.default_rng(1)  # test_dp_math_strict.py::test_exp_bits_equal_libm
    return pad(np.concatenate([
        -rng.uniform(0, 50, 6_000_000), -rng.uniform(0, 50, 2_000_000) * rng.uniform(0, 1, 2_000_000) ** 3,
        -rng.uniform(0, 800, 1_500_000), -10.0 ** rng.uniform(-300, 3.2, 500_000),
        [0.0, -0.0, -1e-320, -2.0 ** -54, -2.0 ** -55, -511.99999, -512.0, -512.0000001, -708.3, -708.5, -744.9, -745.2, -1023.9,
         -1024.0, -1e300, -np.inf, -0.6931471805599453, -1.0],
        -rng.uniform(0, 760, 500_000),
        -10.0 ** rng.uniform(-320, -16, 20_000), neighbours([-2.0 ** -54, -2.0 ** -53], 3),   # |x| < 2^-54: 1 + x
        neighbours([-512.0], 50), -rng.uniform(511, 513, 100_000),                           # the specialcase switch
        -rng.uniform(708, 745.2, 200_000), neighbours([-708.3964185322641, -745.1332191019411, -745.2], 20),  # denormal results
        -rng.uniform(1024, 1e4, 1000), neighbours([-1024.0], 5), [-1e10, -1.7976931348623157e308, -np.inf]]))


def log1p_strict_args():
    rng = np.random.default_rng(2)  # test_dp_math_strict.py::test_log1p_bits_equal_libm
    hi_word = lambda h: np.array([h << 32], dtype=np.uint64).view(np.float64)  # noqa: E731
    return pad(np.concatenate([
        rng.uniform(0, 1, 4_000_000), np.exp(-rng.uniform(0, 50, 4_000_000)), np.exp(-rng.uniform(0, 2, 2_000_000)),
        np.exp(-rng.uniform(0, 800, 500_000)), 1.0 - 10.0 ** rng.uniform(-16, -3, 500_000),
        [0.0, 1.0, 2.0 ** -54, 2.0 ** -29, np.nextafter(2.0 ** -29, 0), np.nextafter(2.0 ** -54, 0), 5e-324,
         0.41421353816986084, np.nextafter(0.41421353816986084, 0), 0.41421356237309503, 0.4142135623730951, 0.5,
         np.nextafter(1.0, 0), 1.0 - 2.0 ** -20, 1.0 - 2.0 ** -19, 1.0 - 2.0 ** -21],
        # fdlibm's branch points: hx = 0x3FDA827A (k = 0 below), 0x3e200000 (2^-29), 0x3c900000 (2^-54); 1 + x at sqrt 2 (the
        # normalisation of u switches at hu = 0x6a09e) and at 2; |f| < 2^-20 (1 + x within 2^-20 of 1 or 2)
        neighbours(np.concatenate([hi_word(0x3FDA827A), hi_word(0x3e200000), hi_word(0x3c900000)]), 20),
        np.clip(neighbours([2.0 ** 0.5 - 1.0, np.array([0x3ff6a09e << 32], dtype=np.uint64).view(np.float64)[0] - 1.0], 200), 0, 1),
        np.clip(neighbours([1.0, 0.5, 0.25], 50), 0, 1), 1.0 - 2.0 ** -rng.uniform(18, 53, 20_000), 2.0 ** -rng.uniform(18, 60, 20_000),
        # denormal e
        np.arange(0, 64) * 5e-324, np.ldexp(rng.uniform(0.5, 1, 20_000), rng.integers(-1074, -1021, 20_000)), [2.2250738585072014e-308]]))


def log_plus_strict_args():
    rng = np.random.default_rng(3)  # test_dp_math_strict.py::test_log_plus_bits_equal_reference_expression
    n = 7 * 600_000
    x = rng.uniform(-60000, 50, n)
    y = x + np.where(rng.random(n) < 0.5, rng.uniform(-45, 45, n), rng.standard_normal(n) * 10.0 ** rng.uniform(-9, 3, n))
    x[:7] = [-np.inf, -np.inf, 3.0, -5.0, 0.0, 0.0, -7.25]
    y[:7] = [-np.inf, -2.5, -np.inf, -5.0, -600.0, -720.0, -7.25]
    # DP-like pairs: |hi| from 1e-3 to 1e6, hi - lo from 0 to 60, either order
    m = 1_000_000
    hi = -10.0 ** rng.uniform(-3, 6, m)
    lo = hi - rng.uniform(0, 60, m)
    swap = rng.random(m) < 0.5
    eq = -10.0 ** rng.uniform(-3, 6, 10_000)                       # equal operands
    one = -10.0 ** rng.uniform(-3, 6, 1000)
    ninf, nan = np.full(1000, -np.inf), np.full(1000, np.nan)
    xs = np.concatenate([x, np.where(swap, lo, hi), eq, one, ninf, ninf, one, nan, nan, ninf, nan])
    ys = np.concatenate([y, np.where(swap, hi, lo), eq, ninf, one, ninf, nan, one, nan, nan, ninf])
    return pad(xs, ys)


def usable_stdevs():
    sd = _model_stdevs()  # test_division_by_constant_equals_ieee_division; a significand of all ones is refused at model load
    return sd[(sd.view(np.uint64) & np.uint64(0x000fffffffffffff)) != np.uint64(0x000fffffffffffff)]


def pdf_strict_args():
    rng = np.random.default_rng(4)  # test_certified_emission_bits_equal_reference_expression
    n = 7 * 300_000
    mean = rng.standard_normal(n) * 2
    sd = rng.choice(usable_stdevs(), n)
    x = mean + sd * rng.standard_normal(n) * rng.choice([0.1, 1.0, 6.0, 40.0], n)
    # every stdev with dividends x - mean = 0, 2^-53 |x| (x a power of two, mean the double below it), one ulp, and up to 1e300
    s = np.tile(usable_stdevs(), 8)
    k = len(s)
    x2 = np.ldexp(1.0, rng.integers(-8, 9, k)) * rng.choice([-1.0, 1.0], k)
    big = rng.choice([-1.0, 1.0], k) * 10.0 ** rng.uniform(0, 300, k)
    big[:16] = [1e300, -1e300] * 8
    xe = np.concatenate([x2, x2, x2 * rng.uniform(1, 2, k), big])
    me = np.concatenate([x2, np.nextafter(x2, 0), np.zeros(k), rng.standard_normal(k) * 2])
    me[2 * k:3 * k] = np.nextafter(xe[2 * k:3 * k], np.inf)
    x, mean, sd = np.concatenate([x, xe]), np.concatenate([mean, me]), np.concatenate([sd, np.tile(s, 4)])
    x, mean, sd = pad(x, mean, sd)
    return x, mean, sd, 1.0 / sd, -np.log(sd)   # 1 / sd: IEEE division, RN(1 / stdev) as the model load forms it


def softplus_edges():
    """d on the table's nodes, on the ties of the magic-number rounding, around -40 and at 0 -- each with its neighbours"""
    i = np.arange(0, 5121)
    return np.concatenate([neighbours(-i / 128.0, 2), neighbours(-(2 * i[:-1] + 1) / 256.0, 2), neighbours([-40.0], 40),
                           [0.0, -0.0, -39.999, -40.01, -41.0, -1e9, -1e300, -np.inf, -5e-324, -1e-300]])


def softplus_args():
    rng = np.random.default_rng(3)  # test_dp_math.py::_grid7
    d = np.concatenate([_grid7(rng), softplus_edges(), -rng.uniform(0, 45, 600_000), -np.abs(rng.standard_normal(300_000)) * 3,
                        -10.0 ** rng.uniform(-12, 1.7, 100_000)])
    return pad(np.minimum(d, 0.0))


def log_plus_args():
    rng = np.random.default_rng(4)  # test_dp_math.py::test_table_logplus_special_values_and_oracle, scaled up
    n = 900_000
    a = rng.uniform(-5000, 100, n)
    b = a + rng.uniform(-60, 60, n)
    d = softplus_edges()
    base = -np.floor(rng.uniform(0, 4096, len(d)))      # integers: base + d is exact for every edge value
    inf = np.inf
    xs = np.concatenate([a, np.zeros(len(d)), d, base, base + d, [-inf, 3.0, -inf, -5.0, 1e4, -2000.0, 0.25, np.nan, 1.0, np.nan]])
    ys = np.concatenate([b, d, np.zeros(len(d)), base + d, base, [-inf, -inf, -7.5, -5.0, 1e4 - 800.0, 2000.0, 0.25, 1.0, np.nan, np.nan]])
    return pad(xs, ys)


def emission_args(n=7 * 150_000):
    rng = np.random.default_rng(3)  # test_dp_math.py::test_kernel_emission_within_a_few_ulp_of_the_reference_expression
    x = rng.standard_normal(n) * 3
    mean = rng.standard_normal(n)
    sd = rng.uniform(0.05, 0.5, n)
    sd[: n // 2] = 0.15
    x[:100] = mean[:100] + 40 * sd[:100]                      # far tails
    x[100:200] = mean[100:200]                                # the mode
    x, mean, sd = pad(x, mean, sd)
    return x, mean, sd, 1.0 / sd, -np.log(sd)


def exp128_args():
    rng = np.random.default_rng(5)  # test_dp_math.py::test_exp_table128_vec_accuracy_and_exact_zero
    d = np.concatenate([-rng.uniform(0, 60, 3500), -rng.uniform(600, 708, 1400), rng.uniform(-1e-9, 1e-9, 700), rng.uniform(0, 5, 686),
                        -rng.uniform(708, 746, 700), [0.0, -745.0, -745.2, -999.0, -1e9, 1e-300, -1e-300, -0.5, -np.inf, np.nan, -746.0, -750.0, -751.0, -1e300]])
    return pad(np.concatenate([
        d, rng.uniform(-760, 1, 1_000_000), -rng.uniform(745.0, 760, 20_000), neighbours([-745.1332191019411, -750.0, -708.3964185322641], 50),
        np.full(64, np.nan), np.full(64, -np.inf),
        np.arange(0, 200) * 2.0 ** -54, rng.uniform(0, 1e-12, 20_000), -np.arange(0, 200) * 2.0 ** -54, [1.0, np.nextafter(1.0, 0)]]))


# ---- step 3: device bits == host bits ------------------------------------------------------------------------------------
def test_exp_strict_bits(cm):
    x = exp_strict_args()
    want, = cm.h("ev_exp_strict", [x], 1)
    got, = cm.run(OP_EXP_STRICT, [x], 1)
    assert_same_bits("exp_strict_vec<7>", got, want, [x])
    # glibc's exp table left in global memory: the same bits
    got_g, = cm.run(OP_EXP_STRICT, [x[:P * 2000]], 1, lds=False)
    assert_same_bits("exp_strict_vec<7>, table in global memory", got_g, got[:P * 2000], [x], "global", "LDS")


def test_log1p_strict_bits(cm):
    x = log1p_strict_args()
    want, = cm.h("ev_log1p_strict", [x], 1)
    got, = cm.run(OP_LOG1P_STRICT, [x], 1)
    assert_same_bits("log1p_strict_vec<7>", got, want, [x])


def test_log_plus_strict_bits(cm):
    """log_plus_strict_vec<7>, and log_plus_strict_from on the (hi, diff) log_plus_issue hands the fallback. A NaN operand
    reaches max_hw (v_max_f64 on the device, fmax on the host): the expectation is what the host build gives."""
    x, y = log_plus_strict_args()
    want, want_from = cm.h("ev_log_plus_strict", [x, y], 2)
    got, got_from = cm.run(OP_LOG_PLUS_STRICT, [x, y], 2)
    assert_same_bits("log_plus_strict_vec<7>", got, want, [x, y])
    assert_same_bits("log_plus_strict_from", got_from, want_from, [x, y])
    ok = ~(np.isnan(x) | np.isnan(y))
    assert_same_bits("log_plus_strict_from vs log_plus_strict_vec", got_from[ok], got[ok], [x[ok], y[ok]], "from", "vec")
    if cm.libm_is_restated_glibc:
        ref, = cm.h("ev_ref_log_plus", [x, y], 1)
        assert_same_bits("log_plus_strict_vec<7> vs x + log1p(exp(y - x))", got[ok], ref[ok], [x[ok], y[ok]], "device", "libm")


def test_strict_emission_and_quotients_bits(cm):
    """The reference's emission with hipcc's real division, the two certified forms (recip_lo formed on the device) and the
    three quotients behind them: equal to each other, to the host build, and to the device's own a / b."""
    x, mean, sd, inv, nls = pdf_strict_args()
    names = ["log_normal_pdf_strict", "log_normal_pdf_cert_vec<7>", "emission_vec<ARITH_STRICT> (cert4)", "div_by_const",
             "div_by_const4", "a / b"]
    want = cm.h("ev_pdf_strict", [x, mean, sd, inv, nls], 6)
    got = cm.run(OP_PDF_STRICT, [x, mean, sd, inv, nls], 6)
    for name, g, w in zip(names, got, want):
        assert_same_bits(name, g, w, [x, mean, sd])
    for k in (1, 2):
        assert_same_bits(names[k] + " vs " + names[0], got[k], got[0], [x, mean, sd], "certified", "division")
    for k in (3, 4):
        assert_same_bits(names[k] + " vs the device's a / b", got[k], got[5], [x, mean, sd], "constant", "division")
    assert np.array_equal(got[5][np.isfinite(got[5])], ((x - mean) / sd)[np.isfinite(got[5])])  # IEEE division, by numpy's


def test_default_log_plus_bits(cm):
    """log_plus_issue<7> + log_plus_finish<7> (default arithmetic) and + log_plus_finish3<7>: d on the nodes -i/128, on the
    ties -(2i+1)/256 of the magic-number rounding, either side of -40, 0."""
    x, y = log_plus_args()
    want5, want3 = cm.h("ev_log_plus_table", [x, y], 2)
    got5, got3 = cm.run(OP_LOG_PLUS, [x, y], 2)
    assert_same_bits("log_plus_issue<7> + log_plus_finish<7>", got5, want5, [x, y])
    assert_same_bits("log_plus_issue<7> + log_plus_finish3<7>", got3, want3, [x, y])
    # the softplus nodes left in global memory: the same bits
    g5, g3 = cm.run(OP_LOG_PLUS, [x, y], 2, lds=False)
    assert_same_bits("log_plus_finish<7>, table in global memory", g5, got5, [x, y], "global", "LDS")
    assert_same_bits("log_plus_finish3<7>, table in global memory", g3, got3, [x, y], "global", "LDS")


def test_table_softplus_bits_and_accuracy(cm):
    """softplus_table_vec<7> / softplus_table3_vec<7>: the host build's bits, and the bounds test_dp_math.py asserts of the host
    build (1.5e-16 and 1.3e-12 absolute against 40-digit mpmath) on the device's own results."""
    d = softplus_args()
    want5, want3 = cm.h("ev_softplus_table", [d], 2)
    got5, got3 = cm.run(OP_SOFTPLUS, [d], 2)
    assert_same_bits("softplus_table_vec<7>", got5, want5, [d])
    assert_same_bits("softplus_table3_vec<7>", got3, want3, [d])
    assert np.all(got5[d <= -40.0] == 0.0) and np.all(got3[d <= -40.0] == 0.0)   # d <= -40 -> exactly 0
    mp.mp.dps = 40
    pick = np.concatenate([np.arange(4200), np.random.default_rng(7).choice(len(d), 15_000, replace=False)])  # _grid7 first
    worst5 = worst3 = mp.mpf(0)
    for i in pick:
        t = mp.log1p(mp.exp(mp.mpf(float(d[i]))))
        worst5 = max(worst5, abs(mp.mpf(float(got5[i])) - t))
        worst3 = max(worst3, abs(mp.mpf(float(got3[i])) - t))
    assert worst5 < 1.5e-16, worst5
    assert worst3 < 1.3e-12, worst3


def test_default_emission_bits(cm):
    x, mean, sd, inv, nls = emission_args()
    want, = cm.h("ev_pdf_vec", [x, mean, inv, nls], 1)
    got, = cm.run(OP_PDF, [x, mean, inv, nls], 1)
    assert_same_bits("emission_vec<ARITH_DEFAULT> (log_normal_pdf_vec<7>)", got, want, [x, mean, sd])


def test_exp_table128_bits_and_accuracy(cm):
    """exp_table128_vec<7> and min_hw(., 1.0) behind it (forward_train_chain): the host build's bits; an exact 0 below -745.2
    and for NaN / -inf; never above 1 after the clip; 2.5e-12 relative against 40-digit mpmath (test_dp_math.py's bound)."""
    x = exp128_args()
    want, want_min = cm.h("ev_exp128", [x], 2)
    got, got_min = cm.run(OP_EXP128, [x], 2)
    assert_same_bits("exp_table128_vec<7>", got, want, [x])
    assert_same_bits("min_hw(exp_table128_vec<7>, 1.0)", got_min, want_min, [x])
    g, g_min = cm.run(OP_EXP128, [x], 2, lds=False)   # 2^(i/128) left in global memory: the same bits
    assert_same_bits("exp_table128_vec<7>, table in global memory", g, got, [x], "global", "LDS")
    assert_same_bits("min_hw(., 1.0), table in global memory", g_min, got_min, [x], "global", "LDS")
    assert np.all(got[~np.isfinite(x) | (x < -745.14)] == 0.0)
    assert np.all(got_min <= 1.0) and np.any(got > 1.0) and np.all(got_min[got > 1.0] == 1.0)
    assert np.any((got > 1.0) & (got < 1.0 + 1e-12))   # results that round to just above 1 are in the set
    mp.mp.dps = 40
    tiny = mp.mpf(2) ** -1074
    worst = 0.0
    pick = np.concatenate([np.arange(7000), np.random.default_rng(8).choice(len(x), 13_000, replace=False)])
    for i in pick:
        if not np.isfinite(x[i]) or x[i] < -745.14:
            continue
        t = mp.exp(mp.mpf(float(x[i])))
        if t > mp.mpf(2) ** -1022:
            worst = max(worst, float(abs(mp.mpf(float(got[i])) - t) / t))
        else:
            assert abs(mp.mpf(float(got[i])) - t) <= tiny * mp.mpf("0.51") + t * mp.mpf("3e-12"), (x[i], got[i])
    assert worst < 2.5e-12, worst


def test_folded_emission_bits(cm):
    """set_emis<ARITH_FOLDED> + emission_vec<ARITH_FOLDED>, the training sweeps' folded emission: bit-equal to the same product,
    difference, product and FMA on the host."""
    x, mean, sd, inv, nls = emission_args()
    want, = cm.h("ev_emis_folded", [x, mean, inv, nls], 1)
    got, = cm.run(OP_EMIS_FOLDED, [x, mean, inv, nls], 1)
    assert_same_bits("set_emis<ARITH_FOLDED> + emission_vec<ARITH_FOLDED>", got, want, [x, mean, sd])


def test_folded_emission_accuracy(cm):
    """The folded emission against ln N(x; mean, stdev) in 40-digit mpmath (mp.dps = 40) on 20 000 samples, by the measure and
    the bound test_dp_math.py::test_kernel_emission_within_a_few_ulp_of_the_reference_expression applies to the 5-operation
    emission: 4 ulp of the terms the result adds up.

    This test changed the kernels. The two-FMA form they ran, u = fma(x, c, -RN(mean c)), missed the bound: 5.093 ulp
    (mp.dps = 40) at x = 0x1.3e3bc8aec515bp+0, mean = 0x1.b36d21cbe9105p+0, stdev = 0.15. It carries the rounding of mean c,
    half an ulp of |mean| c and not of |u|, times 2 |u|: an error that grows with |mean| / stdev. With the difference first,
    u = (x - mean) c (one operation more), the worst case of the same samples is 3.382 ulp."""
    x, mean, sd, inv, nls = emission_args()
    x, mean, sd, inv, nls = (v[:P * 45] for v in (x, mean, sd, inv, nls))   # 20 160 cells; far tails and the mode come first
    got, = cm.run(OP_EMIS_FOLDED, [x, mean, inv, nls], 1)
    mp.mp.dps = 40
    half_log_2pi = mp.log(2 * mp.pi) / 2
    worst, at = 0.0, None
    for i in range(20_000):
        xi, mi, si = mp.mpf(float(x[i])), mp.mpf(float(mean[i])), mp.mpf(float(sd[i]))
        z = (xi - mi) / si
        exact = -z * z / 2 - mp.log(si) - half_log_2pi
        scale = np.spacing(0.5 * ((x[i] - mean[i]) / sd[i]) ** 2 + abs(np.log(sd[i])) + 0.92)
        e = float(abs(mp.mpf(float(got[i])) - exact)) / scale
        if e > worst:
            worst, at = e, (float(x[i]).hex(), float(mean[i]).hex(), float(sd[i]).hex())
    print("folded emission: worst error %.3f ulp of its terms at (x, mean, stdev) = %s" % (worst, at))
    assert worst <= 4.0, (worst, at)


# ---- step 4: the certified logPlus as the kernels run it -------------------------------------------------------------------
def dp_like_pairs(n, seed):
    """tests/test_dp_math_strict.py's cert_log_plus, in numpy: |hi| log-uniform in [1e-3, 1e6] (now and then 0 or tiny), d of
    its three kinds, either order"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-3, 6, n)
    hi = -mag
    r = rng.integers(0, 1024, n)
    hi[r == 0] = 0.0
    hi[r == 1] = mag[r == 1] * 1e-12
    kind = rng.integers(0, 3, n)
    d = np.where(kind == 0, -45.0 * rng.uniform(0, 1, n), np.where(kind == 1, -3.0 * rng.uniform(0, 1, n) ** 4, -10.0 ** rng.uniform(-12, 2, n)))
    lo = hi + d
    swap = rng.random(n) < 0.5
    return np.where(swap, lo, hi), np.where(swap, hi, lo)


def host_cert(cm, x, y):
    amb = np.zeros(len(x), dtype=np.uint8)
    want, lo = cm.h("ev_log_plus_cert", [x, y], 2, extra=[amb])
    return want, lo, amb.astype(bool)


def expected_fallbacks(amb):
    """per wave: the registers in which some lane's certificate failed"""
    return amb.reshape(-1, 64, 7).any(axis=1).sum(axis=1)


def test_certified_log_plus_on_dp_like_pairs(cm):
    n = P * 11_200   # 5 017 600 pairs
    x, y = dp_like_pairs(n, 21)
    want, _, amb = host_cert(cm, x, y)
    got, fb = cm.run(OP_LOG_PLUS_CERT, [x, y], 1, fallbacks=True)
    assert 0.01 < amb.mean() < 0.6   # both paths are exercised
    assert_same_bits("log_plus_issue<7> + log_plus_finish_certified", got, want, [x, y], "device", "host log_plus_cert")
    assert np.array_equal(fb, expected_fallbacks(amb))
    if cm.libm_is_restated_glibc:
        ref, = cm.h("ev_ref_log_plus", [x, y], 1)
        assert_same_bits("log_plus_finish_certified vs x + log1p(exp(y - x))", got, ref, [x, y], "device", "libm")


@pytest.fixture(scope="module")
def crafted(cm):
    """Rows (waves of 64 lanes x 7 registers) in which the ambiguous cells sit where the fallback's register selection can go
    wrong. Which cells ARE ambiguous is the host build's verdict (log_plus_finish_cert<1>), taken on the finished arrays."""
    rng = np.random.default_rng(31)
    # pools: |hi| <~ 8 (the certificate's interval spans several ulp of the sum: often ambiguous), |hi| >= 1e3 (it holds)
    m = 400_000
    hi_s = -rng.uniform(0.05, 8.0, m)
    xs, ys = hi_s, hi_s - rng.uniform(0, 3, m) ** 2
    want_s, lo_s, amb_s = host_cert(cm, xs[: m // 7 * 7], ys[: m // 7 * 7])
    up = np.flatnonzero(amb_s & differing(want_s, lo_s))   # ambiguous, and the sum is NOT the certificate's lower end
    dn = np.flatnonzero(amb_s & ~differing(want_s, lo_s))  # ambiguous, and it is
    hi_l = -10.0 ** rng.uniform(3, 6, m)
    xl, yl = hi_l, hi_l - rng.uniform(0, 45, m)
    _, _, amb_l = host_cert(cm, xl[: m // 7 * 7], yl[: m // 7 * 7])
    sure = np.flatnonzero(~amb_l)
    assert len(up) > 1000 and len(dn) > 1000 and len(sure) > 100_000

    rows = []   # each: list of (lane, register, "up" | "dn")
    lanes = [0, 63, 29]
    for j in range(7):                       # one register alone, in lane 0, lane 63, an interior lane
        for ln in lanes:
            rows.append([(ln, j, "up")])
    for j in range(7):                       # two registers together: in the same lane, and in different ones
        for k in range(j + 1, 7):
            rows.append([(11, j, "up"), (11, k, "up")])
            rows.append([(0, j, "up"), (63, k, "up"), (40, k, "dn")])
    rows.append([(5, j, "up") for j in range(7)])                          # all seven, one lane
    rows.append([(9 * j, j, "up") for j in range(7)] + [(63, 3, "dn")])    # all seven, seven lanes
    rows += [[] for _ in range(8)]                                          # none
    for _ in range(60):                      # random subsets of registers, random lanes, some lanes twice
        regs = np.flatnonzero(rng.random(7) < 0.4)
        row = []
        for j in regs:
            l_up, l_dn = (int(v) for v in rng.choice(64, 2, replace=False))
            row.append((l_up, int(j), "up"))
            if rng.random() < 0.5:
                row.append((l_dn, int(j), "dn"))
        rows.append(row)
    n = len(rows) * P
    fill = rng.choice(sure, n)
    x, y = xl[fill].copy(), yl[fill].copy()
    for r, row in enumerate(rows):
        for ln, j, kind in row:
            src = rng.choice(up if kind == "up" else dn)
            x[r * P + ln * 7 + j], y[r * P + ln * 7 + j] = xs[src], ys[src]
    flip = rng.random(n) < 0.5   # either operand order
    x, y = np.where(flip, y, x), np.where(flip, x, y)
    want, lo, amb = host_cert(cm, x, y)
    return x, y, want, lo, amb


def test_certified_log_plus_picks_the_ambiguous_registers(cm, crafted):
    x, y, want, lo, amb = crafted
    a = amb.reshape(-1, 64, 7)
    regs = a.any(axis=1)                         # [row][register]
    # coverage, on the host's classification, before any device result is looked at
    for j in range(7):
        only = regs[:, j] & (regs.sum(axis=1) == 1)
        assert only.any(), "no row in which register %d alone is ambiguous" % j
        for ln in (0, 63):
            assert (only & a[:, ln, j]).any(), (j, ln)
        assert (only & a[:, 1:63, j].any(axis=1)).any(), j
        for k in range(j + 1, 7):
            assert (regs[:, j] & regs[:, k] & (regs.sum(axis=1) == 2)).any(), "registers %d and %d never ambiguous together" % (j, k)
    assert regs.all(axis=1).any() and (~regs.any(axis=1)).any()
    got, fb = cm.run(OP_LOG_PLUS_CERT, [x, y], 1, fallbacks=True)
    assert_same_bits("log_plus_finish_certified, crafted rows", got, want, [x, y], "device", "host log_plus_cert")
    assert np.array_equal(fb, regs.sum(axis=1))


# ---- step 5: the comparisons above can fail ----------------------------------------------------------------------------------
def test_a_build_without_the_fallback_is_caught(cm, crafted):
    """-DDYN_EXP_NO_CERT_FALLBACK keeps the certificate's lower sum where the certificate failed: on the crafted rows every
    ambiguous (row, register) then holds a cell that differs from the host's log_plus_cert (each was given at least one cell
    whose sum is not the lower end), and the differing cells are exactly those the host predicts."""
    x, y, want, lo, amb = crafted
    got, fb = cm.run(OP_LOG_PLUS_CERT, [x, y], 1, lib=cm.nofb, fallbacks=True)
    bad = differing(got, want)
    regs = amb.reshape(-1, 64, 7).any(axis=1)
    assert regs.sum() > 100
    assert np.array_equal(bad.reshape(-1, 64, 7).any(axis=1), regs)    # at least one per ambiguous (row, register), none elsewhere
    assert np.array_equal(bad, differing(lo, want))
    assert np.array_equal(fb, regs.any(axis=1).astype(np.uint32))      # this build counts rows


def test_a_contracted_build_is_caught(cm):
    """-ffp-contract=fast in place of off: hipcc then fuses the a * b + c the headers leave unfused on purpose, and the strict
    functions leave the host build's bits. On an MI355X (ROCm 7), of 224 000 arguments each: exp_strict_vec 41 (only below
    -512: scale + scale * tmp of exp_strict_special), log1p_strict_vec 2 490, log_plus_strict_vec 192, log_normal_pdf_strict
    and both certified emissions 27 511 each ((-0.5 q) q + neg_log_stdev); the quotients div_by_const, div_by_const4 and
    a / b do not change (they are written as FMAs already)."""
    rng = np.random.default_rng(41)
    n = P * 500
    differs = {}
    x = -rng.uniform(0, 760, n)
    differs["exp_strict_vec"] = int(differing(cm.run(OP_EXP_STRICT, [x], 1, lib=cm.fast)[0], cm.h("ev_exp_strict", [x], 1)[0]).sum())
    e = rng.uniform(0, 1, n)
    differs["log1p_strict_vec"] = int(differing(cm.run(OP_LOG1P_STRICT, [e], 1, lib=cm.fast)[0], cm.h("ev_log1p_strict", [e], 1)[0]).sum())
    a, b = dp_like_pairs(n, 42)
    differs["log_plus_strict_vec"] = int(differing(cm.run(OP_LOG_PLUS_STRICT, [a, b], 2, lib=cm.fast)[0], cm.h("ev_log_plus_strict", [a, b], 2)[0]).sum())
    args = [v[:n] for v in pdf_strict_args()]
    got, want = cm.run(OP_PDF_STRICT, args, 6, lib=cm.fast), cm.h("ev_pdf_strict", args, 6)
    for k, name in enumerate(["log_normal_pdf_strict", "log_normal_pdf_cert_vec", "log_normal_pdf_cert4_vec", "div_by_const", "div_by_const4", "a / b"]):
        differs[name] = int(differing(got[k], want[k]).sum())
    print("results of %d that differ under -ffp-contract=fast: %s" % (n, differs))
    assert any(differs.values()), differs
    # the two whose unfused a * b + c sits on the common path (Lp2 + z Lp3 ...; (-0.5 z) z + neg_log_stdev)
    assert differs["log1p_strict_vec"] and differs["log_normal_pdf_strict"], differs
