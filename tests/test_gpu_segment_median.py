"""The posterior-median kernels (segment_kernels.hpp: k_median, k_median_long, k_final) pinned bit for bit.

`probability` is the median of a segment's per-row path posteriors pp[], and pp[] never leaves the device: the rest of the
suite sees these kernels only through |got - oracle| <= 1e-6 on whole reads, where the order statistics around the middle
lie within 1e-8 of each other on most segments ("What the end-to-end check cannot see"). Two parts:

  1. tests/device_math/segment_median.hip, compiled with the product's flags, hands the product's own launches path arrays
     built on the host (tests/segment_median_cases.py) and every output bit -- rows, med_hi, med_lo, the poison where
     nothing may be written -- is compared with a sort. Not GPU-marked: that the harness compiles, that the batch has the
     shape launch.cpp gives it, and that the inputs can tell a wrong selection from the right one (four deliberately wrong
     references, computed on the CPU, must each differ in a short and in a long segment of every value family).
  2. Three homopolymer reads through Aligner.align_batch on which a one-rank error moves `probability` by 10 x the
     tolerance or more; the premise is asserted on the CPU oracle (tests/path_posteriors.py), not GPU-marked.

No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import segment_median_cases as smc
from conftest import ROOT
from dynamont_amd import _native, synth
from path_posteriors import homopolymer_reads, median, path_posteriors

gpu = pytest.mark.gpu

PROB_TIGHT = 1e-6   # tests/test_gpu_parity.py
ROW = np.dtype([("signal_pos", "<u4"), ("sequence_pos", "<u4"), ("probability", "<f8")])   # nt_kernels.hpp, SegRow
LAYOUTS = ["seg_off_by_read", "seg_off_by_order"]   # host_prepare's (by read index); ascending in processing order
FAMILY_CASES = ["%s/%s/%d" % k for k in smc.family_segments()]


@pytest.fixture(scope="module")
def harness_so(tmp_path_factory):
    """tests/device_math/segment_median.hip -> a shared library, with the flags of every translation unit of the product"""
    so = tmp_path_factory.mktemp("segmed") / "libsegmed.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/segment_median.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(so)


@pytest.fixture(scope="module")
def batches():
    b = {"seg_off_by_read": smc.build_batch("read"), "seg_off_by_order": smc.build_batch("order")}
    for x in b.values():
        for a in (x.pp, x.pathn, x.segrow, x.path_off, x.seg_off, x.T, x.N, x.read, x.status):
            a.setflags(write=False)
    return b


@pytest.fixture(scope="module")
def want(batches):
    return {k: b.reference() for k, b in batches.items()}


def run_on_device(lib, b):
    """sm_run -> med_hi, med_lo and the rows, n_seg + GUARD entries each; every HIP call must have returned hipSuccess"""
    n_out = b.n_seg + smc.GUARD
    hi, lo, rows = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out, dtype=ROW)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.sm_run(C.c_int(len(b.read)), p(b.path_off), p(b.seg_off), p(b.T), p(b.N), p(b.read), C.c_int(len(b.status)), p(b.status),
                   C.c_uint64(b.rows_total), p(b.pp), p(b.pathn), C.c_uint64(b.n_seg), p(b.segrow), C.c_int(smc.KMER_SIZE),
                   C.c_int(smc.POISON), C.c_uint64(n_out), p(hi), p(lo), p(rows), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    return dict(med_hi=hi, med_lo=lo, probability=rows["probability"].copy(), signal_pos=rows["signal_pos"].copy(),
                sequence_pos=rows["sequence_pos"].copy())


@pytest.fixture(scope="module")
def got(harness_so, batches):
    """every layout run twice on the device"""
    lib = C.CDLL(harness_so)
    lib.sm_run.restype = C.c_int
    return {k: [run_on_device(lib, b), run_on_device(lib, b)] for k, b in batches.items()}


def as_bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def mismatch(b, got, want, slots):
    """text for the output slots (of `slots`) whose bits differ, or None"""
    slots = np.asarray(slots)
    lines = []
    for name in ("signal_pos", "sequence_pos", "probability", "med_hi", "med_lo"):
        g, w = as_bits(got[name])[slots], as_bits(want[name])[slots]
        for s in slots[g != w][:5]:
            lines.append("%s[%d]: device %#x, reference %#x" % (name, s, int(as_bits(got[name])[s]), int(as_bits(want[name])[s])))
    return "; ".join(lines) or None


def check_case(batches, got, want, case, layout="seg_off_by_read"):
    b = batches[layout]
    i, j, slot = b.where(case)
    L = len(b.reads[i]["segments"][j])
    for run in (0, 1):
        bad = mismatch(b, got[layout][run], want[layout], [slot])
        assert bad is None, "%s (read %d, segment %d of %d, %d rows, run %d): %s" % (case, i, j, len(b.reads[i]["segments"]), L, run, bad)


# ---- not GPU-marked ----------------------------------------------------------------------------------------------------------
def test_harness_compiles_with_the_products_flags(harness_so):
    assert os.path.getsize(harness_so) > 0


def test_batch_is_built_as_launch_builds_it(batches):
    """The shape of the batch, before any device result is looked at."""
    for layout, b in batches.items():
        n = len(b.read)
        assert 290 <= n <= 450 and b.rows_total % 256 != 0 and b.rows_total < 1_000_000
        assert sorted(b.read.tolist()) == [i for i, r in enumerate(b.reads) if r["desc"]]       # a permutation ...
        assert (b.read != np.arange(n)).sum() > n // 2                                          # ... that is not the identity
        assert (np.diff(b.path_off.astype(np.int64)) == b.T[:-1]).all() and b.path_off[0] == 0  # ascending in processing order
        so = b.seg_off.astype(np.int64)
        assert (np.diff(so) > 0).all() == (layout == "seg_off_by_order")
        assert any(not r["desc"] for r in b.reads)                                              # rows nobody has a descriptor for
        failed = np.flatnonzero(b.status[b.read] != 0)
        assert failed[0] == 0 and failed[-1] == n - 1 and ((failed > 0) & (failed < n - 1)).sum() >= 2
        assert all(np.isnan(b.pp[int(o)]) for o in b.path_off) and np.isnan(b.pp).sum() == n    # row 0 of every read, only
        for k in range(n):                                                                       # pathn and segrow agree
            po, so_k, T, N = int(b.path_off[k]), int(b.seg_off[k]), int(b.T[k]), int(b.N[k])
            col = b.pathn[po + 1:po + T] & 0x7fffffff
            assert col[0] == 1 and col[-1] == N - 1 and (np.diff(col.astype(np.int64)) >= 0).all()
            first = np.flatnonzero(b.pathn[po + 1:po + T] >> 31) + 1
            assert np.array_equal(first, b.segrow[so_k:so_k + N - 1])
        lens = lambda i: np.array([len(s) for s in b.reads[i]["segments"]])  # noqa: E731
        assert b.T.min() == 2 and (b.N == 2).sum() >= 5
        for where, at in (("first", 0), ("index300", 300), ("last", 599)):
            i, j, _ = b.where("shape/600_segments/long_%s" % where)
            assert j == at and len(lens(i)) == 600 and np.flatnonzero(lens(i) > smc.MEDIAN_SHORT_MAX).tolist() == [at]
        i, _, _ = b.where("shape/no_long_segment")
        i2, _, _ = b.where("shape/several_long/0")
        assert lens(i).max() == smc.MEDIAN_SHORT_MAX and (lens(i2) > smc.MEDIAN_SHORT_MAX).sum() == 3
        for L in smc.LENGTHS:
            for pos, (j_want, n_want) in zip(smc.POSITIONS, ((0, 3), (1, 3), (2, 3))):
                i, j, _ = b.where("len/%d/%s" % (L, pos))
                assert j == j_want and len(lens(i)) == n_want and lens(i)[j] == L
    assert set(smc.FAMILIES) >= {"uniform", "all_equal", "two_values", "tie_runs", "exp_fp32", "low_byte", "exponent_only",
                                 "ff_bytes", "zero_denormal", "ordered"}


def test_value_families_hold_what_they_are_named_for():
    seg = smc.family_segments()
    fam = lambda f: {k: v for k, v in seg.items() if k[0] == f}  # noqa: E731
    for f in smc.FAMILIES:   # odd and even lengths on both sides of the split
        Ls = {k[2] for k in fam(f)}
        assert {255, 256, 257, 258} <= Ls, (f, Ls)
    one = np.concatenate(list(fam("exp_fp32").values()))
    assert (one > 1.0).any() and (one[one > 1.0] < 1.002).all() and (one == 1.0).sum() > 100
    below = one[(one < 1.0) & (one > 1.0 - 1e-14)]
    assert len(below) > 100 and len(np.unique(below)) < len(below) // 2                       # heavy ties at 1 - k ulp
    for v in fam("low_byte").values():
        assert len(np.unique(smc.bits(v) >> np.uint64(8))) == 1 and len(np.unique(v)) >= min(len(v) - 1, 256)
    for v in fam("exponent_only").values():
        assert not (smc.bits(v) & np.uint64(0x000fffffffffffff)).any() and v.max() <= 1.0
    assert min(v.min() for v in fam("exponent_only").values()) < 1e-295
    for (_, name, L), v in fam("ff_bytes").items():
        m = smc.bits(np.array([smc.order_stats(v)[0]]))[0]                                    # the median itself carries the 0xff
        pos = {"byte0": [0], "byte3": [3], "byte6": [6], "bytes0-5": range(6)}[name.split("_")[0]]
        assert all((int(m) >> (8 * p)) & 0xff == 0xff for p in pos), (name, L, hex(int(m)))
    z = fam("zero_denormal")
    assert all(0.0 in z[("zero_denormal", "lowest", L)] and 5e-324 in z[("zero_denormal", "lowest", L)] for L in (255, 258))
    assert all(v.max() < 2.3e-308 for v in z.values())
    for L in (256, 258):                                                                        # both branches of the even rule
        for name, same in (("mid-1", True), ("mid", False), ("mid+1", True)):
            hi, lo, _ = smc.order_stats(seg[("two_values", name, L)])
            assert (hi == lo) == same and hi == (0.25 if name == "mid+1" else 0.75)
    for L in (255, 258):
        assert (np.diff(seg[("ordered", "asc_ties", L)]) >= 0).all() and (np.diff(seg[("ordered", "desc_ties", L)]) <= 0).all()
        assert len(np.unique(seg[("ordered", "asc_ties", L)])) < L // 2


@pytest.mark.parametrize("family", list(smc.FAMILIES))
def test_inputs_tell_a_wrong_selection_apart(family):
    """Four wrong references -- rank mid+1, rank mid-1, the even rule replaced by hi, lo always the largest element below hi --
    computed on the CPU from the reference alone: each must differ bitwise from the right one in at least one short and one
    long segment of the family. (all_equal is exempt by construction: there every one of them must agree.)"""
    seg = {k: v for k, v in smc.family_segments().items() if k[0] == family}
    for wrong in smc.WRONG:
        told = {"short": [], "long": []}
        for (_, variant, L), v in seg.items():
            right, other = smc.order_stats(v)[2], smc.order_stats(v, wrong)[2]
            if smc.bits(np.array([right]))[0] != smc.bits(np.array([other]))[0]:
                told["short" if L <= smc.MEDIAN_SHORT_MAX else "long"].append((variant, L))
        if family in smc.EXEMPT:
            assert not told["short"] and not told["long"], (wrong, told)
        else:
            assert told["short"] and told["long"], (family, wrong, told)


def test_homopolymer_reads_expose_a_one_rank_error(models, oracle_built):
    """The premise of test_homopolymer_reads_against_the_oracle, on the CPU oracle: the median of the rebuilt per-row path
    posteriors IS the oracle's probability (bit for bit), and in at least half of each read's segments the order statistics
    next to the middle one lie more than 10 x PROB_TIGHT away from it."""
    from oracle.pyoracle import Oracle
    orc = Oracle(models["syn5"], synth.PORES["dna_r9"][0])
    kinds = set()
    for r in homopolymer_reads(models["syn5"]):
        segs, res = path_posteriors(orc, r.signal, r.sequence)
        med = np.array([median(v) for v in segs])
        assert np.array_equal(med.view(np.uint64), res["probabilities"].view(np.uint64))
        far = 0
        for v in segs:
            s, mid = np.sort(v), len(v) // 2
            right = smc.order_stats(v)[2]
            moved = min(abs(smc.order_stats(v, "rank_up")[2] - right), abs(smc.order_stats(v, "rank_down")[2] - right))
            far += min(s[mid] - s[mid - 1], s[mid + 1] - s[mid], moved) > 10 * PROB_TIGHT
            kinds.add((len(v) > smc.MEDIAN_SHORT_MAX, len(v) & 1))
        print("%d bases: segments of %d..%d rows, medians %.3f..%.3f, %d of %d with both neighbours > 1e-5 away" % (
            len(r.sequence), min(map(len, segs)), max(map(len, segs)), med.min(), med.max(), far, len(segs)))
        assert 2 * far >= len(segs), (far, len(segs))
    assert kinds == {(True, 0), (True, 1), (False, 0), (False, 1)}   # both kernels, both parities


@pytest.fixture(scope="module")
def sliced():
    return smc.build_sliced_batch()


@pytest.fixture(scope="module")
def sliced_want(sliced):
    return smc.reference_sliced(sliced)


def test_sliced_batch_and_its_reference(sliced, sliced_want):
    """65 541 descriptors of T = 3 .. 6, N = 2 .. 3; the vectorised reference equals order_stats() segment by segment on a
    sample; and a second launch of k_median_long / k_final that is handed the first descriptors again (descs in place of
    descs + r0) shows: no row of descriptors 65 535 .. 65 540 is written, one of them holds a 301-row segment."""
    b, s = sliced, sliced.sliced
    n = len(b.read)
    assert n == smc.SLICE + smc.TAIL and sorted(b.read.tolist()) == list(range(n))
    bulk = np.ones(n, dtype=bool)
    bulk[s["long_reads"]] = False
    Tr, Nr = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    Tr[b.read], Nr[b.read] = b.T, b.N
    assert set(Tr[bulk].tolist()) == {3, 4, 5, 6} and set(Nr[bulk].tolist()) == {2, 3}
    assert np.array_equal(np.sort(b.read[smc.SLICE:]), s["tail"]) and (b.status[s["tail"]] == 0).all() and (b.status != 0).sum() == 300
    long_segs = np.flatnonzero(s["seg_len"] > smc.MEDIAN_SHORT_MAX)
    assert s["seg_len"][long_segs].tolist() == [300, 301]
    assert s["seg_read"][long_segs[0]] in b.read[:smc.SLICE] and s["seg_read"][long_segs[1]] in b.read[smc.SLICE:]
    rng = np.random.default_rng(3)
    ok = np.flatnonzero(b.status[s["seg_read"]] == 0)
    for i in np.concatenate([rng.choice(ok, 400, replace=False), long_segs]):
        hi, lo, p = smc.order_stats(s["vals"][s["seg_first"][i]:s["seg_first"][i] + s["seg_len"][i]])
        assert smc.bits(sliced_want["med_hi"][i:i + 1])[0] == smc.bits(np.array([hi]))[0]
        assert smc.bits(sliced_want["probability"][i:i + 1])[0] == smc.bits(np.array([p]))[0]
        if lo is not None:
            assert smc.bits(sliced_want["med_lo"][i:i + 1])[0] == smc.bits(np.array([lo]))[0]
        else:
            assert sliced_want["med_lo"][i] == hi or smc.bits(sliced_want["med_lo"][i:i + 1])[0] == smc.POISON_U64
    failed = np.flatnonzero(b.status[s["seg_read"]] != 0)
    assert (sliced_want["signal_pos"][failed] == smc.POISON_U32).all() and (smc.bits(sliced_want["probability"])[failed] == smc.POISON_U64).all()
    other = smc.reference_sliced(b, skip_descs=np.arange(smc.SLICE, n))
    rows_of_tail = np.flatnonzero(np.isin(s["seg_read"], s["tail"]))
    assert len(rows_of_tail) >= smc.TAIL + 3                                  # one segment at least per read, three in one
    for name in ("signal_pos", "sequence_pos", "probability", "med_hi"):
        assert (as_bits(other[name])[rows_of_tail] != as_bits(sliced_want[name])[rows_of_tail]).all(), name


# ---- on the device -----------------------------------------------------------------------------------------------------------
@gpu
def test_more_reads_than_one_launch_slice(native_lib, harness_so, sliced, sliced_want):
    """65 541 descriptors through launch_segment_medians: k_median_long and k_final run a second launch over descriptors
    65 535 .. 65 540. Every output slot of the batch, bit for bit."""
    other = smc.reference_sliced(sliced, skip_descs=np.arange(smc.SLICE, len(sliced.read)))   # a second launch handed descs, not descs + r0
    assert all((as_bits(other[name]) != as_bits(sliced_want[name])).sum() >= smc.TAIL + 3 for name in ("signal_pos", "probability", "med_hi"))
    lib = C.CDLL(harness_so)
    lib.sm_run.restype = C.c_int
    got = run_on_device(lib, sliced)
    bad = mismatch(sliced, got, sliced_want, np.arange(sliced.n_seg + smc.GUARD))
    assert bad is None, bad


@gpu
@pytest.mark.parametrize("position", smc.POSITIONS)
@pytest.mark.parametrize("length", smc.LENGTHS)
def test_segment_length(batches, got, want, length, position):
    check_case(batches, got, want, "len/%d/%s" % (length, position))


@gpu
@pytest.mark.parametrize("case", FAMILY_CASES)
def test_value_family(batches, got, want, case):
    check_case(batches, got, want, "fam/" + case)


@gpu
@pytest.mark.parametrize("case", ["T=2", "one_segment/2", "one_segment/256", "one_segment/257", "one_segment/300",
                                  "600_segments/long_first", "600_segments/long_first/short_neighbour",
                                  "600_segments/long_index300", "600_segments/long_index300/short_neighbour",
                                  "600_segments/long_last", "600_segments/long_last/short_neighbour",
                                  "no_long_segment", "several_long/0", "several_long/2", "several_long/3"])
def test_read_shape(batches, got, want, case):
    check_case(batches, got, want, "shape/" + case)


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_whole_batch_bit_for_bit(batches, got, want, layout):
    """Every output slot of every read: rows (exact integers, the double's bits), med_hi, med_lo where it is written (even
    lengths; the long kernel also writes it for odd ones), and the poison everywhere else -- rows of failed reads, rows no
    descriptor points at, med_lo of short odd segments, the guard behind the last segment. A second run returns the same."""
    b = batches[layout]
    every = np.arange(b.n_seg + smc.GUARD)
    first, second = got[layout]
    bad = mismatch(b, first, want[layout], every)
    assert bad is None, bad
    for name in first:
        assert np.array_equal(as_bits(first[name]), as_bits(second[name])), name
    assert not np.isnan(first["probability"][:b.n_seg]).any()   # row 0 of a read (NaN) is in no segment


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_failed_reads_keep_the_poison(batches, got, layout):
    b = batches[layout]
    n = 0
    for i, r in enumerate(b.reads):
        if r["status"] == 0:
            continue
        s = slice(int(b.read_seg_off[i]), int(b.read_seg_off[i]) + len(r["segments"]))
        for run in got[layout]:
            assert (run["signal_pos"][s] == smc.POISON_U32).all() and (run["sequence_pos"][s] == smc.POISON_U32).all(), i
            for name in ("probability", "med_hi", "med_lo"):
                assert (as_bits(run[name])[s] == smc.POISON_U64).all(), (i, name)
        n += 1
    assert n >= 8


@gpu
def test_homopolymer_reads_against_the_oracle(models, native_lib, oracle_built):
    """Reads on which the product itself would show a wrong rank (test_homopolymer_reads_expose_a_one_rank_error): segments of
    396-402 rows (k_median_long, both parities) and 82-84 rows (k_median) whose middle order statistics lie 1e-5 .. 1.5e-3
    apart. All-tie reads: they take the certified arithmetic, so the borders are the oracle's."""
    from dynamont_amd import Aligner
    from oracle.pyoracle import Oracle
    reads = homopolymer_reads(models["syn5"])
    al = Aligner(models["syn5"], "dna_r9", device=0)
    res = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
    orc = Oracle(models["syn5"], synth.PORES["dna_r9"][0])
    assert (res.status == 0).all()
    for i, r in enumerate(reads):
        got_i, want_i = res.read(i), orc.align(r.signal, r.sequence, True)
        assert np.array_equal(got_i["sequence_positions"], want_i["sequence_positions"]), i
        assert np.array_equal(got_i["signal_positions"], want_i["signal_positions"]), i
        assert abs(got_i["Z"] - want_i["Z"]) <= 1e-9 * max(1.0, abs(want_i["Z"])), i
        d = np.abs(got_i["probabilities"] - want_i["probabilities"])
        print("%d bases: max |probability - oracle| = %.3g" % (len(r.sequence), d.max()))
        assert d.max() <= PROB_TIGHT, (i, d.max())
    al.close()
