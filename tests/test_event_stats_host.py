"""CPU: the host half of the per-segment signal levels (ABI 9). The native formatter with level columns writes the bytes of
utils.segmentation_to_string(levels=...) -- Python's f"{x:.6f}" for any finite value, in a buffer of exactly the bound --
and without them the bytes of dyn_format_csv; the NumPy restatement of the definition agrees with NumPy's statistics."""
import ctypes as C

import numpy as np
import pytest

from dynamont_amd import Aligner, synth
from dynamont_amd import _native as N
from dynamont_amd._dynamont import AlignBatchResult, _ptr, format_csv
from dynamont_amd.segmentation.utils import segmentation_to_string

pytestmark = pytest.mark.usefixtures("native_lib")

SPECIAL = [-1e-9, -0.0, 0.0, 5e-324, -5e-324, 1e20, -1e20, 1e300, -1e300, 1.7976931348623157e308, 511.9999995, 512.0000005,
           0.0000005, -0.0000005, 0.0000015, 1e15, 1e15 - 0.5, 999999999999999.9] + [k / 128 for k in range(-300, 300, 7)]


# ---- the definition, restated (as tests/test_gpu_event_stats.py) ----
def _chunked(v):
    sums = np.array([np.add.accumulate(v[c:c + 64])[-1] for c in range(0, len(v), 64)])
    return np.add.accumulate(sums)[-1]


def levels_of(x, sp):
    x = np.asarray(x, dtype=np.float64)
    bounds = [int(s) for s in sp] + [len(x)]
    out = np.zeros((3, len(sp)))
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        seg = x[a:b]
        L = len(seg)
        mean = _chunked(seg) / np.float64(L)
        d = seg - mean
        s = np.sort(seg)
        med = s[L // 2] if L % 2 else (s[L // 2 - 1] + s[L // 2]) / 2.0
        out[:, i] = (mean, np.sqrt(_chunked(d * d) / np.float64(L)), med + 0.0)
    return out


def test_restatement_agrees_with_numpy():
    rng = np.random.default_rng(11)
    x = rng.normal(0.3, 1.2, 30000)
    sp = np.concatenate([[0], np.sort(rng.choice(np.arange(1, 29000), 300, replace=False)), [29500]])
    lv = levels_of(x, sp)
    bounds = list(sp) + [len(x)]
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        seg = x[a:b]
        assert abs(lv[0, i] - np.mean(seg)) <= 1e-12 * max(1.0, abs(np.mean(seg)))
        assert abs(lv[1, i] - np.std(seg)) <= 1e-12
        assert lv[2, i] == np.median(seg)
    assert levels_of(np.array([-0.0, 0.0]), [0])[2, 0].hex() == "0x0.0p+0"   # no -0.0 median
    assert levels_of(np.array([2.5]), [0])[:, 0].tolist() == [2.5, 0.0, 2.5]


def test_abi_version(tmp_path):
    al = Aligner(synth.write_model(str(tmp_path / "syn5.model"), 5, seed=7, stdev=0.25), "dna_r9", device="host")
    info = N.DynInfo()
    assert N.lib().dyn_aligner_info(al._h, C.byref(info)) == 0 and info.abi_version >= 9
    al.close()


def _fake_result(rng, n_reads, values):
    """an AlignBatchResult with rows as the GPU fills them, and level columns holding `values` (cycled)"""
    nseg = rng.integers(1, 30, n_reads)
    cap = int(nseg.sum())
    res = AlignBatchResult(n_reads, cap)
    res.seg_offsets[1:] = np.cumsum(nseg)
    res.n_segments[:] = nseg
    res.status[2] = 3   # a failed read: no rows
    res.n_segments[2] = 0
    seqs = []
    for i in range(n_reads):
        a, m = int(res.seg_offsets[i]), int(nseg[i])
        seqs.append("".join(rng.choice(list("ACGT"), m + 4)))
        res.sequence_positions[a:a + m] = np.arange(m) + 2
        res.signal_positions[a:a + m] = np.cumsum(rng.integers(1, 40, m)) - 1
        res.probabilities[a:a + m] = rng.random(m)
    res.states[:] = ord("M")
    res.level_mean, res.level_stdv, res.level_median = (np.resize(np.asarray(values, dtype=np.float64), cap) for _ in range(3))
    res.level_stdv = np.roll(res.level_stdv, 5)
    res.level_median = np.roll(res.level_median, 11)
    return res, seqs


def _python_rows(res, seqs, rid, sid, starts, last, k, rna, levels):
    out = []
    for i in range(res.n):
        if res.status[i] != 0:
            out.append(b"")
            continue
        a, b = int(res.seg_offsets[i]), int(res.seg_offsets[i]) + int(res.n_segments[i])
        d = {"sequence_positions": res.sequence_positions[a:b], "signal_positions": res.signal_positions[a:b],
             "probabilities": res.probabilities[a:b], "states": ["M"] * (b - a)}
        lv = (res.level_mean[a:b], res.level_stdv[a:b], res.level_median[a:b]) if levels else None
        out.append(segmentation_to_string(d, rid[i], sid[i], starts[i], last[i], seqs[i], k, rna, levels=lv))
    return b"".join(out)


@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna004", 9)])
def test_native_rows_equal_python_rows(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    rng = np.random.default_rng(5)
    values = SPECIAL + list(rng.normal(0, 1, 200)) + list(rng.normal(0, 1, 50) * 1e6)
    n = 12
    res, seqs = _fake_result(rng, n, values)
    rid = [f"r{i}" for i in range(n)]
    sid = [f"s{i}" for i in range(n)]
    starts = [int(x) for x in rng.integers(0, 100, n)]
    last = [starts[i] + int(res.signal_positions[int(res.seg_offsets[i]) + max(0, int(res.n_segments[i]) - 1)]) + 50 for i in range(n)]
    rna = pore.startswith("rna")
    want = _python_rows(res, seqs, rid, sid, starts, last, k, rna, True)
    buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
    assert bytes(buf[:int(end[-1])]) == want
    # exactly the bound as capacity, through the C entry points themselves
    L = N.lib()
    ev = N.DynEventOut(_ptr(res.level_mean, N.c_double_p), _ptr(res.level_stdv, N.c_double_p), _ptr(res.level_median, N.c_double_p),
                       res.cap)
    rids = (C.c_char_p * n)(*[x.encode() for x in rid])
    sids = (C.c_char_p * n)(*[x.encode() for x in sid])
    bound = int(L.dyn_format_csv_bound_events(al._h, n, C.byref(res._c), C.byref(ev), rids, sids))
    out = np.zeros(bound, dtype=np.uint8)
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seqs])
    so = np.array(starts, dtype=np.int64)
    li = np.array(last, dtype=np.int64)
    b0 = np.zeros(n, dtype=np.uint64)
    e0 = np.zeros(n, dtype=np.uint64)
    rc = L.dyn_format_csv_events(al._h, n, C.byref(res._c), C.byref(ev), "".join(seqs).encode(), _ptr(seq_off, N.c_u64_p), rids, sids,
                                 so.ctypes.data_as(C.POINTER(C.c_int64)), li.ctypes.data_as(C.POINTER(C.c_int64)), 2,
                                 out.ctypes.data, bound, _ptr(b0, N.c_u64_p), _ptr(e0, N.c_u64_p))
    assert rc == 0
    assert b"".join(bytes(out[int(b0[i]):int(e0[i])]) for i in range(n)) == want
    # ev = NULL: the bytes of dyn_format_csv
    plain = _python_rows(res, seqs, rid, sid, starts, last, k, rna, False)
    res.level_mean = res.level_stdv = res.level_median = None
    buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
    assert bytes(buf[:int(end[-1])]) == plain
    assert int(L.dyn_format_csv_bound_events(al._h, n, C.byref(res._c), None, rids, sids)) == \
        int(L.dyn_format_csv_bound(al._h, n, C.byref(res._c), rids, sids))
    al.close()
