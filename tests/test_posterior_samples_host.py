"""CPU: the host half of posterior path sampling (dyn_aligner_set_posterior_samples). The new symbols resolve, the switch is
range-checked and refused where it cannot work, dyn_format_csv_samples writes the K starts of a row as one field (with
sm == NULL the bytes of dyn_format_csv_borders) and its bound holds, the sink knows its new flag and still refuses the unassigned
ones, the CLI parses its two options. The yardstick of the GPU tests (tests/posterior_sample_cases.py) is held against the
per-border marginals it must reproduce: with 1 024 samples per read the share of samples that put a border on the called row, and
within two rows of it, stays within five standard deviations of border_probability / border_window_probability; no sample
dies; rounding every log-posterior to fp32 changes no path; and four deliberately wrong versions each draw other paths.
(The refusals that need a job -- rescale, auto guide, guide rescue, a guided batch, a fetch from a batch that did not sample --
need a device: tests/test_gpu_posterior_samples.py holds them.)"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import border_confidence_cases as bcc
import posterior_sample_cases as psc
from conftest import ROOT
from dynamont_amd import Aligner, MultiAligner, synth, zstd_io
from dynamont_amd import _native as N
from dynamont_amd._dynamont import _ptr, format_csv
from test_border_confidence_host import _fake_result, _python_rows

pytestmark = pytest.mark.usefixtures("native_lib")


def test_symbols_and_constants(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    declared = set(re.findall(r"\b(dyn_[a-z0-9_]+)\s*\(", hdr))
    for name in ("dyn_aligner_set_posterior_samples", "dyn_batch_fetch_samples", "dyn_format_csv_samples",
                 "dyn_format_csv_bound_samples"):
        assert name in declared and name in N.SIGNATURES
        assert getattr(native_lib, name) is not None
    assert "typedef struct dyn_sample_out" in hdr and "DYN_POSTERIOR_SAMPLES_MAX 64" in hdr
    assert "DYN_CSV_POSTERIOR_SAMPLES 0x10u" in hdr and "DYN_ABI_VERSION 10" in hdr
    assert re.search(r"int dyn_aligner_set_posterior_samples\(dyn_aligner\* a, int count, uint64_t seed\);", hdr)
    assert re.search(r"int dyn_batch_fetch_samples\(dyn_batch\* b, dyn_sample_out\* out\);", hdr)
    for text in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0xFFFFFFFF"):   # the definition is in the header
        assert text in hdr, text
    assert N.DYN_CSV_POSTERIOR_SAMPLES == 16 and N.DYN_POSTERIOR_SAMPLES_MAX == 64 and N.DYN_SAMPLE_DEAD == psc.DEAD
    assert [f[0] for f in N.DynSampleOut._fields_] == ["sample_start", "sample_dead", "capacity", "n", "count"]


def test_switch_range_and_refusals_on_a_host_handle(models):
    al = Aligner(models["syn9"], "rna004", device="host")
    assert al._posterior_samples == (0, 0)
    for bad in (-1, 65):
        with pytest.raises(ValueError, match=r"dyn_aligner_set_posterior_samples: count must be 0 \.\. 64, got " + str(bad)):
            al.set_posterior_samples(bad)
    assert al._posterior_samples == (0, 0)
    for ok, seed in ((0, 0), (1, 5), (64, 2 ** 64 - 1), (0, 0)):
        al.set_posterior_samples(ok, seed)
        assert al._posterior_samples == (ok, seed)
    L = N.lib()
    assert L.dyn_aligner_set_posterior_samples(None, 1, 0) == N.DYN_ERR_INVALID_ARGUMENT
    s, d = np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    assert L.dyn_batch_fetch_samples(None, C.byref(N.DynSampleOut(_ptr(s, N.c_u32_p), _ptr(d, N.c_u32_p), 4, 1, 1))) == \
        N.DYN_ERR_INVALID_ARGUMENT
    # not together with the band retry (the other order needs a device: tests/test_gpu_posterior_samples.py)
    al.set_posterior_samples(4)
    with pytest.raises(ValueError, match="set_band_retry with set_posterior_samples"):
        al.set_band_retry(2)
    al.close()
    assert not hasattr(MultiAligner, "set_posterior_samples")     # as for every per-border rider: no such switch there


@pytest.mark.parametrize("mode", ["ntk", "resquiggle"])
def test_refused_on_an_ntk_handle(models, mode):
    al = Aligner(models["syn9"], "rna004", mode=mode, device="host")
    with pytest.raises(ValueError, match="dyn_aligner_set_posterior_samples: modes ntk / resquiggle"):
        al.set_posterior_samples(4)
    al.set_posterior_samples(0)
    assert al._posterior_samples == (0, 0)
    al.close()


# ---- the formatter ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pore,k", [("dna_r9", 5), ("rna004", 9)])
def test_native_rows_carry_the_samples(pore, k, tmp_path):
    model = synth.write_model(str(tmp_path / "m.model"), k, seed=7, stdev=0.2)
    al = Aligner(model, pore, device="host")
    rng = np.random.default_rng(6)
    n, K = 12, 5
    res, seqs, cols = _fake_result(rng, n, list(rng.random(200)))
    rid = [f"r{i}" for i in range(n)]
    sid = [f"s{i}" for i in range(n)]
    starts = [int(x) for x in rng.integers(0, 100, n)]
    last = [starts[i] + int(res.signal_positions[int(res.seg_offsets[i]) + max(0, int(res.n_segments[i]) - 1)]) + 50 for i in range(n)]
    rna = pore.startswith("rna")
    samples = rng.integers(0, 4_000_000_000, (K, res.cap)).astype(np.uint32)
    samples[2, :] = psc.DEAD                                           # a dead sample prints as it is, whatever the read's offset
    samples[0, 0] = 0
    dead = np.zeros(n, dtype=np.uint32)
    L = N.lib()
    rids = (C.c_char_p * n)(*[x.encode() for x in rid])
    sids = (C.c_char_p * n)(*[x.encode() for x in sid])
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off[1:] = np.cumsum([len(s) for s in seqs])
    so, li = np.array(starts, dtype=np.int64), np.array(last, dtype=np.int64)
    bd = N.DynBorderOut(*(_ptr(cols[c], N.c_double_p) for c in ("border_probability", "border_window_probability")), res.cap)
    sm = N.DynSampleOut(_ptr(samples, N.c_u32_p), _ptr(dead, N.c_u32_p), res.cap, n, K)

    def native(bdp, smp, old=False, slack=0):
        if old:
            bound = int(L.dyn_format_csv_bound_borders(al._h, n, C.byref(res._c), None, None, bdp, rids, sids))
        else:
            bound = int(L.dyn_format_csv_bound_samples(al._h, n, C.byref(res._c), None, None, bdp, smp, rids, sids))
        out = np.full(bound + 64, 0x5a, dtype=np.uint8)
        b0, e0 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        tail = ("".join(seqs).encode(), _ptr(seq_off, N.c_u64_p), rids, sids, so.ctypes.data_as(C.POINTER(C.c_int64)),
                li.ctypes.data_as(C.POINTER(C.c_int64)), 2, out.ctypes.data, bound - slack, _ptr(b0, N.c_u64_p), _ptr(e0, N.c_u64_p))
        if old:
            rc = L.dyn_format_csv_borders(al._h, n, C.byref(res._c), None, None, bdp, *tail)
        else:
            rc = L.dyn_format_csv_samples(al._h, n, C.byref(res._c), None, None, bdp, smp, *tail)
        if slack:
            return rc
        assert rc == 0
        assert (out[bound:] == 0x5a).all() and int(e0.max()) <= bound                 # the bound bounds the output
        return b"".join(bytes(out[int(b0[i]):int(e0[i])]) for i in range(n))

    def python(borders):
        rows = _python_rows(res, seqs, rid, sid, starts, last, k, rna, cols, False, False, borders).split(b"\n")[:-1]
        out, j = [], 0
        for i in range(n):
            if res.status[i] != 0:
                continue
            a = int(res.seg_offsets[i])
            for s in range(int(res.n_segments[i])):
                field = ";".join(str(int(v) if v == psc.DEAD else int(v) + starts[i]) for v in samples[:, a + s])
                out.append(rows[j] + b"," + field.encode() + b"\n")
                j += 1
        assert j == len(rows)
        return b"".join(out)

    for borders in (False, True):
        bdp = C.byref(bd) if borders else None
        assert native(bdp, C.byref(sm)) == python(borders)                             # after the border columns
        assert native(bdp, None) == native(bdp, None, old=True)                       # sm == NULL: dyn_format_csv_borders' bytes
    assert b";4294967295;" in python(False)
    assert native(None, C.byref(sm), slack=1) == N.DYN_ERR_INVALID_ARGUMENT           # too small a buffer: refused
    # the Python wrapper follows the result object's columns
    res.sample_starts, res.sample_dead = samples, dead
    buf, begin, end = format_csv(al, res, seqs, rid, sid, starts, last, threads=3, compact=True)
    assert bytes(buf[:int(end[-1])]) == python(False)
    broken = N.DynSampleOut(None, _ptr(dead, N.c_u32_p), res.cap, n, K)
    assert int(L.dyn_format_csv_bound_samples(al._h, n, C.byref(res._c), None, None, None, C.byref(broken), rids, sids)) == 0
    al.close()


HEADER = b"readid,signalid,start,end,basepos,base,motif,state,posterior_probability,polish"
PARTS = {1: b",level_mean,level_stdv,level_median", 2: b",median_delta,mad_delta,homogeneity",
         8: b",border_probability,border_window_probability", 16: b",sample_starts"}


@pytest.mark.parametrize("flags", [0x10, 0x11, 0x12, 0x18, 0x19, 0x1a, 0x1b])
def test_sink_header(tmp_path, flags):
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    out = str(tmp_path / "o.csv.zst")
    assert L.dyn_csv_sink_open_ex(out.encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags, C.byref(h), err, 1024) == 0, err.value
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    text = zstd_io.decompress(open(out, "rb").read())
    assert text == HEADER + b"".join(PARTS[b] for b in (1, 2, 8, 16) if flags & b) + b"\n"


@pytest.mark.parametrize("flags", [0x20, 0x30, 0x14, 0x4, 0x110])
def test_sink_refuses_unassigned_flags(tmp_path, flags):
    L = N.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    rc = L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1, flags,
                                C.byref(h), err, 1024)
    assert rc == N.DYN_ERR_INVALID_ARGUMENT and b"unknown flags" in err.value and not h.value


def test_cli_flags_parse():
    from dynamont_amd.segmentation.segment import parse
    base = ["-r", "x", "-b", "y", "-o", "z", "--mode", "basic", "-p", "rna004"]
    a = parse(base)
    assert a.posterior_samples == 0 and a.sample_seed == 0
    a = parse(base + ["--posterior-samples", "16", "--sample-seed", "7"])
    assert a.posterior_samples == 16 and a.sample_seed == 7
    assert parse(base + ["--posterior-samples", "4", "--border-confidence", "8"]).border_confidence == 8     # the two combine
    for bad in (["--posterior-samples", "65"], ["--posterior-samples", "4", "--sample-seed", "-1"],
                ["--posterior-samples", "4", "--rescale-iters", "1"], ["--posterior-samples", "4", "--guide-auto", "16"],
                ["--posterior-samples", "4", "--guide-rescue", "16"]):
        with pytest.raises(SystemExit):
            parse(base + bad)


# ---- the yardstick itself --------------------------------------------------------------------------------------------------------
def test_the_random_number_is_the_definitions():
    """SplitMix64 from state 0 gives the published first outputs; u is the top 53 bits"""
    x = np.array([0], dtype=np.uint64)
    assert int(psc.mix(x)[0]) == 0xE220A8397B1DCDAF
    with np.errstate(over="ignore"):
        assert int(psc.mix(x + np.uint64(0x9E3779B97F4A7C15))[0]) == 0x6E789E6AA1B965F4
    seed, i, k, t = 12345, 3, 7, 99

    def m(v):
        z = (v + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return z ^ (z >> 31)
    want = (m((m((m(seed + i) + k) & (2 ** 64 - 1)) + t) & (2 ** 64 - 1)) >> 11) * 2.0 ** -53
    assert psc.uniform(seed, i, np.array([k]), np.array([t]))[0] == want and 0.0 <= want < 1.0
    assert psc.uniform(2 ** 64 - 1, 1, np.array([k]), np.array([t]))[0] == psc.uniform(0, 0, np.array([k]), np.array([t]))[0]   # mod 2^64


@pytest.fixture(scope="module")
def lattices(models, oracle_built):
    """(set name, read) -> (LPM, LPE, oracle result, band), computed once"""
    from oracle.pyoracle import Oracle
    sets = psc.read_sets(models["syn5"])
    orcs, cache = {}, {}

    def get(name, j):
        if (name, j) not in cache:
            pore, band, reads = sets[name]
            if (pore, band) not in orcs:
                orcs[pore, band] = Oracle(models["syn5"], synth.PORES[pore][0], band)
            cache[name, j] = psc.lattices(orcs[pore, band], reads[j].signal, reads[j].sequence, band) + (band,)
        return cache[name, j]
    get.sets = sets
    return get


EVERY_READ = [(name, j) for name, count in (("rna002", 3), ("dna_r9", 3), ("band50", 3), ("band50_long", 1), ("band400_long", 1),
                                            ("wide", 1)) for j in range(count)]


@pytest.mark.parametrize("name,j", EVERY_READ)
def test_marginals_completion_and_fp32(lattices, name, j):
    """1 024 samples of the read: none dies; the share of samples with border j on the called row stays within 5 sigma of
    border_probability, the share within two rows of it within 5 sigma of border_window_probability at W = 2
    (sigma <= sqrt(0.25 / 1024): 0.078 in all); the first 64 samples are the same paths with every log-posterior rounded to fp32;
    at most one of those is undecided."""
    lpm, lpe, res, band = lattices(name, j)
    starts, dead, undecided = psc.walk(lpm, lpe, 5, j, 1024)
    assert not dead.any() and (starts != psc.DEAD).all()
    rows = res["signal_positions"].astype(np.int64)                  # the called starts: M row - 1, the unit of the samples
    bp, bwp = bcc.from_lpm(lpm, rows + 1, 2)
    s = starts.astype(np.int64)
    on_row = (s == rows[None, :]).mean(axis=0)
    near = (np.abs(s - rows[None, :]) <= 2).mean(axis=0)
    bound = 5 * math.sqrt(0.25 / 1024)
    print(f"{name} {j}: T {lpm.shape[0]} N {lpm.shape[1]}: |share - border_probability| <= {np.abs(on_row - bp).max():.4f}, "
          f"window {np.abs(near - bwp).max():.4f} (bound {bound:.4f}); undecided {int(undecided.sum())} of 1024")
    assert np.abs(on_row - bp).max() <= bound and np.abs(near - bwp).max() <= bound
    assert (s[:, 0] == 0).all() and (np.diff(s, axis=1) >= 2).all() and s.max() <= lpm.shape[0] - 3    # paths, each of them
    s32, d32, _ = psc.walk(lpm, lpe, 5, j, 64, fp32=True)
    differs = (s32 != starts[:64]).any(axis=1)
    assert not d32.any() and not (differs & ~undecided[:64]).any()
    psc.check_cap([undecided[:64]], f"{name} {j}")


@pytest.mark.parametrize("wrong", psc.MUTATIONS)
def test_wrong_versions_differ_from_the_yardstick(lattices, wrong):
    """u >= p, column n instead of n + 1, a stream not keyed by k, a start off by one row: on every read set at least one of 16
    paths of the first read differs (and for all but the unkeyed stream, every one)"""
    for name in ("rna002", "dna_r9", "band50", "band50_long", "wide"):
        lpm, lpe, _, _ = lattices(name, 0)
        starts, _, _ = psc.walk(lpm, lpe, 5, 0, 16)
        other, _, _ = psc.walk(lpm, lpe, 5, 0, 16, mutate=wrong)
        differs = (other != starts).any(axis=1)
        assert differs.sum() >= (15 if wrong == "stream_not_keyed_by_k" else 16), (wrong, name, int(differs.sum()))


def test_mutations_can_fail_and_the_stream_is_keyed(lattices):
    """the unmutated yardstick against itself differs by nothing; another read index, sample or seed gives another path"""
    lpm, lpe, _, _ = lattices("dna_r9", 0)
    a, _, _ = psc.walk(lpm, lpe, 5, 0, 16)
    b, _, _ = psc.walk(lpm, lpe, 5, 0, 16, mutate=None)
    assert np.array_equal(a, b)
    assert len({row.tobytes() for row in a}) == 16
    assert not np.array_equal(a, psc.walk(lpm, lpe, 5, 1, 16)[0]) and not np.array_equal(a, psc.walk(lpm, lpe, 6, 0, 16)[0])
    assert np.array_equal(a[:4], psc.walk(lpm, lpe, 5, 0, 4)[0])      # sample k does not depend on K
