"""CPU: the host half of the per-read site calls (dyn_aligner_set_site_calls, dyn_aligner_set_site_model). The header text and the
symbols; what a handle without a device refuses; the footprint of the kernels of tests/device_math/site_calls.hip as the compiler
reports it; the restatement of tests/site_call_cases.py on the built rows, and that those rows tell each WRONG version a kernel
could compute from the definition; the model files of segmentation.utils."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import site_call_cases as scc
import site_mixture_cases as smc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, _native as N
from dynamont_amd._dynamont import AlignBatchResult, JobWants, _OPTIONAL

pytestmark = pytest.mark.usefixtures("native_lib")

SYMBOLS = ("dyn_aligner_set_site_model", "dyn_aligner_site_model_reset", "dyn_aligner_site_model_fetch", "dyn_aligner_set_site_calls",
           "dyn_batch_fetch_site_calls", "dyn_format_csv_calls", "dyn_format_csv_bound_calls")


def test_header_text_and_symbols(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in SYMBOLS:
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    flat = " ".join(hdr.split())
    assert "int dyn_aligner_set_site_calls(dyn_aligner* a, int on);" in flat
    assert "int dyn_batch_fetch_site_calls(dyn_batch* b, dyn_site_call_out* out);" in flat
    assert "typedef struct dyn_site_call_out" in hdr and "#define DYN_CSV_SITE_CALLS 0x800u" in hdr and N.DYN_CSV_SITE_CALLS == 0x800
    assert [f[0] for f in N.DynSiteCallOut._fields_] == ["site_probability", "site_z", "capacity"]
    assert "site_call_kernels.hpp" in N.HEADERS
    assert "calls" in JobWants._fields and [c[0] for c in _OPTIONAL["calls"][0]] == ["site_probability", "site_z"]
    res = AlignBatchResult(2, 5)
    assert res.site_probability is None and res.site_z is None            # off: nothing new on a result


def test_kernels_live_in_one_header_and_one_unit():
    src = lambda f: open(os.path.join(N.CSRC, f)).read()  # noqa: E731
    assert len(re.findall(r"__global__", src("site_call_kernels.hpp"))) == 4        # k_scall_short, k_scall_long, the model's scatter and gather
    assert len(re.findall(r"__global__", src("site_summary_kernels.hpp"))) == 2      # the table's kernels are as they were
    users = [f for f in os.listdir(N.CSRC) if '#include "site_call_kernels.hpp"' in src(f)]
    assert users == ["site_summary.hip"]
    text = src("site_call_kernels.hpp")
    assert "sm_find_or_insert" not in text.split("k_scall_long")[1].split("k_site_model_scatter")[0]   # the call kernels only find
    assert "sm_estep<1>" in text and "__shfl" not in text and "atomicAdd(ms.dropped" in text


def test_entry_points_refuse_what_they_cannot_serve(native_lib, models):
    z = np.zeros(1)
    p = z.ctypes.data_as(N.c_double_p)
    assert native_lib.dyn_aligner_set_site_calls(None, 1) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_set_site_model(None, 0, 1, p, p, p, p, p, None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_model_reset(None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_aligner_site_model_fetch(None, 0, 1, p, p, p, p, p) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_batch_fetch_site_calls(None, None) == N.DYN_ERR_INVALID_ARGUMENT
    al = Aligner(models["syn9"], "rna004", device="host")
    assert native_lib.dyn_aligner_set_site_model(al._h, 0, 1, None, p, p, p, p, None) == N.DYN_ERR_INVALID_ARGUMENT
    m = {k: np.zeros(3) for k in scc.COLUMNS}
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.set_site_model(0, m)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.site_model(0, 0)
    with pytest.raises(RuntimeError, match="no GPU bound"):
        al.reset_site_model()
    with pytest.raises(ValueError, match="the columns of the model differ in length"):
        al.set_site_model(0, dict(m, var1=np.zeros(2)))
    with pytest.raises(ValueError, match="status and the columns of the model differ in length"):
        al.set_site_model(0, dict(m, status=np.zeros(2, dtype=np.uint32)))
    # the switch without the per-site table: refused before the device is looked at, for every kind of job
    al.set_site_calls(True)
    assert al._job_wants(True).calls is True and al._job_wants(False) == JobWants()
    sig, seq = [np.zeros(200)], ["ACGT" * 10]
    with al.batch(sig, seq) as b:
        with pytest.raises(ValueError, match=r"dyn_batch_align: dyn_aligner_set_site_calls is on, which needs dyn_aligner_set_site_summary\(a, num_sites > 0\)"):
            b.align(True)
        for job in (lambda: b.align(False), b.train):
            with pytest.raises(ValueError, match=r"dyn_aligner_set_site_calls is on, which scores the rows of align\(calc_probabilities = 1\) jobs alone"):
                job()
    al.set_site_calls(False)
    assert al._job_wants(True).calls is None and not any(al._job_wants(True))
    with al.batch(sig, seq) as b:
        with pytest.raises(RuntimeError, match="no GPU bound"):
            b.align(True)
    al.close()
    for call in (lambda: MultiAligner.set_site_calls(None, True), lambda: MultiAligner.set_site_model(None, 0, m)):
        with pytest.raises(NotImplementedError, match="use one Aligner per device"):
            call()


def test_kernels_compile_with_the_products_flags_beside_a_resident_workgroup(tmp_path):
    """tests/device_math/site_calls.hip builds for gfx950 with the product's flags; the compiler's resource remarks show the two call
    kernels and the model's two window kernels without scratch, within 13 KB of static LDS and 152 VGPRs"""
    cmd = [N.hipcc_path()] + N.hipcc_flags() + ["-I", N.CSRC, "-Rpass-analysis=kernel-resource-usage", "-shared", "-x", "hip",
                                                 os.path.join(ROOT, "tests", "device_math", "site_calls.hip"), "-o", str(tmp_path / "libsc.so")]
    assert "-ffp-contract=off" in cmd and "--offload-arch=gfx950" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    blocks = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", r.stderr, re.S)
    vgprs = dict(re.findall(r"Function Name: (\S+).*? VGPRs: (\d+)", r.stderr, re.S))
    seen = {}
    for k in ("k_scall_short", "k_scall_long", "k_site_model_scatter", "k_site_model_gather"):
        hit = [(n, int(s), int(l)) for n, s, l in blocks if k in n]
        assert len(hit) == 1, (k, [n for n, _, _ in blocks])
        seen[k] = (hit[0][1], hit[0][2], int(vgprs[hit[0][0]]))
    print(seen)
    for k, (scratch, lds, v) in seen.items():
        assert scratch == 0 and lds <= 13 * 1024 and v <= 152, (k, scratch, lds, v)
    assert seen["k_scall_short"][1] >= 2048 and seen["k_scall_long"][1] >= 4096      # the exp table is staged into LDS in both


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    b = scc.build_batch()
    n = len(b.reads)
    prob, z = scc.reference(b.reads, scc.MODEL, scc.NUM_SITES, 0, n)
    return b, prob, z


def rows_of(b, site, long_rows=None):
    out, j = [], 0
    for status, segs in b.reads:
        for s, x in segs:
            if s == site and status == 0 and (long_rows is None or (len(x) > scc.SHORT_MAX) == long_rows):
                out.append(j)
            j += 1
    return out


def test_the_restatement_on_the_built_rows(built):
    b, prob, z = built
    nan = lambda v: scc.bits(v) == scc.NAN_BITS  # noqa: E731
    assert prob.size == z.size == b.sites.size == sum(len(segs) for _, segs in b.reads)
    lens = np.array([len(x) for _, segs in b.reads for _, x in segs])
    assert {1, 255, 256, 257, 16385 + 64} <= set(lens.tolist())
    # no id, an id outside the table, an unset row: no call
    for s in (scc.NONE, scc.NUM_SITES, scc.NONE - 1, scc.UNSET, 12, 13, 14, scc.NUM_SITES - 1):
        r = rows_of(b, s)
        assert len(r) >= 2 and nan(prob[r]).all() and nan(z[r]).all(), s
    # a one-component row: site_z alone, in both kernels
    for s in scc.ONE_COMPONENT:
        for long_rows in (False, True):
            r = rows_of(b, s, long_rows)
            assert r and nan(prob[r]).all() and np.isfinite(z[r]).all(), (s, long_rows)
    # a two-component row: both, the probability inside [0, 1]
    r = rows_of(b, scc.SHORT_ONLY)
    assert len(r) >= 12 and ((prob[r] > 0) & (prob[r] < 1)).all() and np.isfinite(z[r]).all()
    # the exp argument past -512 and -1 024: the special path's tiny values, then the exact +0 and the exact 1
    far = dict(zip(scc.FAR_MEANS, prob[rows_of(b, scc.FAR)]))
    assert 0 < far[42.6] < 1e-315 < far[43.0] < 1e-300 < far[44.9] < 1e-200 and far[102.0] == 1.0
    assert far[40.24] == 0.0 and far[39.0] == 0.0 and far[-2.0] == 0.0
    assert math.copysign(1.0, far[39.0]) == 1.0 and far[50.0] == 0.5 and far[49.9] < 0.5 < far[55.12]
    assert smc.exp_strict(-700.0) > 0 and smc.exp_strict(-1100.0) == 0.0 and smc.exp_strict(0.0) == 1.0
    # q_0 == q_1: the `up = false` side, p_1 / (p_0 + p_1) with both factors 1
    eq = prob[rows_of(b, scc.EQUAL)][:4]
    assert (eq == 0.25).all()
    # m * m reaches 2^64: no call; just below: a call
    two = rows_of(b, scc.TWO)
    big = [j for j in two if abs(scc.event_mean(_row(b, j))) >= 2.0 ** 31 or not math.isfinite(scc.event_mean(_row(b, j)))]
    kept = [j for j in big if abs(scc.event_mean(_row(b, j))) < 2.0 ** 32]
    assert len(big) == 8 and len(kept) == 2 and not nan(z[kept]).any() and nan(z[[j for j in big if j not in kept]]).all()
    assert (z[kept] > 1e10).all() and (prob[kept] == 1.0).all()


def _row(b, j):
    k = 0
    for _, segs in b.reads:
        if j < k + len(segs):
            return segs[j - k][1]
        k += len(segs)
    raise IndexError(j)


@pytest.mark.parametrize("wrong", scc.WRONG)
def test_the_built_rows_tell_a_wrong_version_from_the_definition(built, wrong):
    b, prob, z = built
    n = len(b.reads)
    wp, wz = scc.reference(b.reads, scc.MODEL, scc.NUM_SITES, 0, n, wrong=wrong)
    dp, dz = np.flatnonzero(scc.bits(wp) != scc.bits(prob)), np.flatnonzero(scc.bits(wz) != scc.bits(z))
    sites = b.sites
    lens = np.array([len(x) for _, segs in b.reads for _, x in segs])
    if wrong == "pi0_half":            # pi0 taken as 0.5: every two-component site whose pi1 is not 0.5 moves, site_z stays
        assert dz.size == 0 and dp.size > 100 and {scc.TWO, scc.SHORT_ONLY, scc.EQUAL} <= set(sites[dp].tolist())
    elif wrong == "swapped":
        assert dz.size == 0 and dp.size > 100 and scc.FAR in sites[dp]
    elif wrong == "z_var1":            # site_z formed with var1: the probability stays
        assert dp.size == 0 and dz.size > 100 and scc.TWO in sites[dz] and scc.EQUAL not in sites[dz]   # (var0 == var1 there)
    elif wrong == "value_without_two":  # a value where the row is not two-component
        assert dz.size == 0 and set(sites[dp].tolist()) == {2, 3} and not np.isnan(wp[dp]).any()
    else:                              # the chunk sums in the wrong order: rows above 256 samples alone, m moves and both columns with it
        assert dp.size >= 1 and (lens[dp] > scc.SHORT_MAX).all() and (lens[dz] > scc.SHORT_MAX).all() and set(dp.tolist()) <= set(dz.tolist())
        if wrong == "chunk_wrap":      # the same additions up to 256 chunks: the row of 16 385 + 64 samples alone tells it
            assert lens[dp].tolist() == [16385 + 64]


def test_sparse_reference_drops_the_late_site(built):
    b, prob, z = built
    n = len(b.reads)
    sp, sz = scc.reference(b.reads, scc.MODEL, scc.NUM_SITES, 0, n, present=set(scc.SET_FIRST))
    diff = np.flatnonzero(scc.bits(sp) != scc.bits(prob))
    assert diff.size >= 3 and set(b.sites[diff].tolist()) == {scc.LATE} and (scc.bits(sp[diff]) == scc.NAN_BITS).all()
    assert sorted(s for s, row in scc.MODEL.items() if scc.is_set(row)) == sorted(scc.SET_FIRST + (scc.LATE,))
    assert len(scc.SET_FIRST) == scc.CAPACITY and sum(c for _, c in scc.WINDOWS) == 15


def test_the_ordering_the_whole_read_test_asks_for_holds_with_room_to_spare():
    """tests/test_gpu_site_calls.py asserts that, at the shifted sites, the share of rows called (site_probability >= 0.5) is larger
    among the shifted reads than among the others. Checked here on synthetic event means of that shape with the restatement and
    the mixture restatement: 48 + 48 rows around one level with the spread of the test's reads, two thirds of the second sample
    0.5 higher (tests/test_gpu_site_mixture.py: SHIFT); the fitted model separates them by a wide margin."""
    rng = np.random.default_rng(77)
    spec = (32, -4.0, 4.0)
    margins = []
    for trial in range(20):
        centre, sd = rng.uniform(-1.5, 1.5), rng.uniform(0.05, 0.12)      # the spread of an event mean over ~12 samples at sd <= 0.4
        a = rng.normal(centre, sd, 48)
        shifted = np.arange(48) % 3 != 0
        bvals = rng.normal(centre, sd, 48) + 0.5 * shifted
        fit = smc.fit(smc.histogram(a, *spec), smc.histogram(bvals, *spec), *spec, **smc.DEFAULTS)
        if fit["status"] not in (0, 2):
            continue
        row = tuple(fit[k] for k in scc.COLUMNS)
        called = np.array([scc.call(row, float(m))[0] >= 0.5 for m in bvals])
        base = np.array([scc.call(row, float(m))[0] >= 0.5 for m in a])
        margins.append(called[shifted].mean() - max(called[~shifted].mean(), base.mean()))
    print("called share among the shifted rows minus the larger share elsewhere, per trial:", margins)
    assert len(margins) >= 15 and min(margins) > 0.25 and float(np.median(margins)) > 0.75, margins   # the test asks for > 0


# ---- the model files -----------------------------------------------------------------------------------------------------------------
def test_model_files_hold_the_set_rows_and_refuse_other_contigs(tmp_path):
    from dynamont_amd.segmentation.utils import load_site_model, save_site_model
    n = 50
    m = {k: np.zeros(n) for k in scc.COLUMNS}
    for s, row in ((3, scc.MODEL[scc.TWO]), (17, scc.MODEL[2]), (49, scc.MODEL[scc.FAR])):
        for k, v in zip(scc.COLUMNS, row):
            m[k][s] = v
    m["mu1"][20] = 5.0                                                     # not set (var0 == 0): not stored
    path = str(tmp_path / "model.npz")
    assert save_site_model(path, m, ["chrA", "chrB"], [30, 20], histogram=(32, -4.0, 4.0)) == 3
    got = load_site_model(path, ["chrA", "chrB"], [30, 20])
    assert got["site"].tolist() == [3, 17, 49] and got["histogram"] == (32, -4.0, 4.0) and got["num_sites"] == 50
    for k in scc.COLUMNS:
        assert got[k].tobytes() == m[k][[3, 17, 49]].tobytes()
    dense = got["dense"](0, 50)
    for k in scc.COLUMNS:
        want = m[k].copy()
        want[20] = 0.0
        assert dense[k].tobytes() == want.tobytes()
    assert load_site_model(path)["site"].size == 3                         # no contigs given: nothing to check
    with pytest.raises(ValueError, match="the site model was fitted over other contigs"):
        load_site_model(path, ["chrA", "chrC"], [30, 20])
    with pytest.raises(ValueError, match="the site model was fitted over other contigs"):
        load_site_model(path, ["chrA", "chrB"], [30, 21])
    with pytest.raises(ValueError, match="the columns of the model differ in length"):
        save_site_model(path, dict(m, pi1=np.zeros(3)), ["chrA", "chrB"], [30, 20])
