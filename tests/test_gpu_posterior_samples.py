"""GPU (-m gpu): posterior path sampling (Aligner.set_posterior_samples, sample_kernels.hpp). Whole reads through every place a
lattice lives -- the separate layout (plain and certified reads), the in-place layout, a page-starved pool, the banded-lattice
kernel -- against the NumPy restatement over the CPU oracle's lattices (tests/posterior_sample_cases.py): every decided path
entry for entry, no dead sample, and no more undecided paths than the cap allows. The walk and its accessors also run, compiled
into a test unit with the product's flags, on a lattice the test writes itself (out-of-band slots poisoned, a crafted dead end).
Switching the samples on moves nothing else, and off is the launch it has always been."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import border_confidence_cases as bcc
import posterior_sample_cases as psc
from conftest import ROOT
from dynamont_amd import Aligner, _native, synth, zstd_io

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

SEED = 20261020


@pytest.fixture(scope="module")
def sets(models):
    return psc.read_sets(models["syn5"])


@pytest.fixture(scope="module")
def want(models, sets, oracle_built):
    """yardstick(members, K, seed) -> [(starts, dead, undecided, oracle result)] for a batch made of members = [(set name, index
    in the set)], the read's index in THAT batch keying its stream; the lattices are computed once per read"""
    from oracle.pyoracle import Oracle
    orcs, lats = {}, {}

    def get(members, K, seed=SEED):
        out = []
        for i, (name, j) in enumerate(members):
            pore, band, reads = sets[name]
            if (name, j) not in lats:
                if (pore, band) not in orcs:
                    orcs[pore, band] = Oracle(models["syn5"], synth.PORES[pore][0], band)
                lats[name, j] = psc.lattices(orcs[pore, band], reads[j].signal, reads[j].sequence, band)
            lpm, lpe, res = lats[name, j]
            out.append(psc.walk(lpm, lpe, seed, i, K) + (res,))
        return out
    return get


def members_of(sets, name):
    return [(name, j) for j in range(len(sets[name][2]))]


def run(model, pore, band, reads, K, seed=SEED, budget=None, W=0):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    al.set_posterior_samples(K, seed)
    if W:
        al.set_border_confidence(W)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        b.align(True)
        res = b.fetch()
        tm = b.timing()
    al.close()
    return res, tm


def run_off(model, pore, band, reads, budget=None, W=0):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    if W:
        al.set_border_confidence(W)
    res = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
    assert res.sample_starts is None and res.sample_dead is None and "sample_starts" not in res.read(0)
    al.close()
    return res


def check(res, yard, K, what):
    """every decided path equals the yardstick entry for entry along the oracle's own borders; nothing is dead; the undecided
    paths stay under the cap. Returns their number."""
    assert (res.status[:len(yard)] == 0).all(), (what, res.status)
    assert res.sample_starts.shape[0] == K and res.sample_starts.dtype == np.uint32 and res.sample_dead.dtype == np.uint32
    und = []
    for i, (starts, dead, undecided, orc_res) in enumerate(yard):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        assert m == starts.shape[1] and np.array_equal(res.signal_positions[a:a + m], orc_res["signal_positions"]), (what, i)
        assert not dead.any() and res.sample_dead[i] == 0, (what, i, res.sample_dead[i])
        got = res.sample_starts[:, a:a + m]
        differ = (got != starts).any(axis=1)
        print(f"{what} read {i}: {K} paths of {m} starts, {int(undecided.sum())} undecided, {int(differ.sum())} differ")
        bad = np.nonzero(differ & ~undecided)[0]
        assert bad.size == 0, (what, i, "sample", int(bad[0]), "first entry", int(np.nonzero(got[bad[0]] != starts[bad[0]])[0][0]))
        assert (got != psc.DEAD).all()
        und.append(undecided)
    return psc.check_cap(und, what)


def same_segments(a, b):
    """no segment, Z or probability moved"""
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "probabilities"):
        assert np.array_equal(getattr(a, col)[:m].view(np.uint64), getattr(b, col)[:m].view(np.uint64)), col


def same_samples(a, b):
    m = int(a.seg_offsets[-1])
    assert np.array_equal(a.sample_starts[:, :m], b.sample_starts[:, :m]) and np.array_equal(a.sample_dead, b.sample_dead)


# ---- 1. separate layout, plain and certified reads --------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 7, 64])
@pytest.mark.parametrize("name", ["rna002", "dna_r9"])
def test_separate_layout(models, sets, want, name, K):
    """rna002: pad + A, a structural tie at the read's start -- the launch that carries both arithmetic flavours; dna_r9: the plain
    launch. One lane, a few lanes, the whole wave."""
    pore, band, reads = sets[name]
    res, tm = run(models["syn5"], pore, band, reads, K)
    assert tm["lp_inplace"] == 0 and tm["launches"] == 1
    if name == "rna002":
        assert tm["reads_strict"] == len(reads)
    else:
        assert tm["reads_strict"] == 0
    check(res, want(members_of(sets, name), K), K, f"{name} K={K}")
    d = res.read(1)
    a, m = int(res.seg_offsets[1]), int(res.n_segments[1])
    assert d["sample_starts"].shape == (K, m) and np.array_equal(d["sample_starts"], res.sample_starts[:, a:a + m])
    if K == 7:
        same_segments(res, run_off(models["syn5"], pore, band, reads))


# ---- 2. windows that leave the band; 3. slot aliasing and page crossings -------------------------------------------------------
@pytest.mark.parametrize("name", ["band50", "band50_long", "band400_long"])
def test_narrow_band_and_wrapping_slots(models, sets, want, name):
    """imperfect dna_r9 reads at band 50: the path strays from the diagonal and a sample's neighbours lie outside the band's window.
    The 600-base read has 593 lattice columns: a band slot is n mod 448, so slots wrap and an unmasked read of a slot returns
    another column's value; its 8 647 rows span several pages. At band 400 and at band 50."""
    pore, band, reads = sets[name]
    if name != "band50":
        assert len(reads[0].sequence) - 5 + 2 > 448
    res, _ = run(models["syn5"], pore, band, reads, 16)
    check(res, want(members_of(sets, name), 16), 16, name)


# ---- 4. in-place layout and a page-starved pool --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["inplace", "page_starved"])
@pytest.mark.parametrize("name", ["rna002", "dna_r9", "band50", "band50_long"])
def test_inplace_layout_and_page_starved_pool(models, sets, want, monkeypatch, name, path):
    pore, band, reads = sets[name]
    members = members_of(sets, name)
    budget = None
    if path == "page_starved" and name == "band50_long":
        # one read alone cannot queue for pages: the long read shares its batch, and its pool, with the three reads of 200 bases
        reads = sets["band50"][2] + reads
        members = members_of(sets, "band50") + members
    if path == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    else:
        # a read's lattice takes ~(448 * 8 + 56) bytes per row: room for a fifth of the batch, and for the longest read one and a
        # half times over
        lens = sorted((len(r.signal) for r in reads), reverse=True)
        budget = int(max(0.2 * sum(lens), 1.5 * lens[0]) * (448 * 8 + 56))
    res, tm = run(models["syn5"], pore, band, reads, 16, budget=budget)
    off = run_off(models["syn5"], pore, band, reads, budget)
    if path == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
        assert tm["lp_inplace"] == 1
        if name == "rna002":
            assert tm["reads_strict"] == len(reads)                 # in place AND both flavours: k_read_queue<JOB_ALIGN_INPLACE | JOB_SAMPLE, true>
        if name == "dna_r9":
            assert tm["reads_strict"] == 0                          # ... and the plain in-place launch
    else:
        print(f"{name} page-starved: pool_pages {tm['pool_pages']}, page_rows {tm['page_rows']}, n_static {tm['n_static']} of {len(reads)}")
    check(res, want(members, 16), 16, f"{name} {path}")
    same_segments(res, off)


# ---- 5. the banded-lattice kernel ------------------------------------------------------------------------------------------------
def test_banded_lattice_kernel(models, sets, want):
    """one rna002 read of 600 bases at band = 600: half band 298, above the register sweeps' 223 (band_reads.hip)"""
    pore, band, reads = sets["wide"]
    assert min(band // 2, (len(reads[0].sequence) - 5 + 2) // 2) == 298
    res, _ = run(models["syn5"], pore, band, reads, 16)
    check(res, want(members_of(sets, "wide"), 16), 16, "wide")
    same_segments(res, run_off(models["syn5"], pore, band, reads))
    both, _ = run(models["syn5"], pore, band, reads, 16, W=8)              # ... behind the border phase: the same paths
    same_samples(both, res)
    bd = run_off(models["syn5"], pore, band, reads, W=8)
    m = int(bd.seg_offsets[-1])
    assert np.array_equal(both.border_window_probability[:m].view(np.uint64), bd.border_window_probability[:m].view(np.uint64))


# ---- 6. reproducible, keyed by the seed, the same through a ticket ---------------------------------------------------------------
def test_runs_seeds_and_tickets(models, sets, want):
    pore, band, reads = sets["dna_r9"]
    first, _ = run(models["syn5"], pore, band, reads, 16)
    again, _ = run(models["syn5"], pore, band, reads, 16)
    same_samples(first, again)                                              # two runs: identical bits
    other, _ = run(models["syn5"], pore, band, reads, 16, seed=SEED + 1)
    m = int(first.seg_offsets[-1])
    assert (other.sample_starts[:, :m] != first.sample_starts[:, :m]).any(axis=1).all()     # another seed: every path another
    check(other, want(members_of(sets, "dna_r9"), 16, SEED + 1), 16, "dna_r9 seed + 1")
    al = Aligner(models["syn5"], pore, band=band, device=0)
    al.set_posterior_samples(16, SEED)
    t = al.align_async(*synth.pack_reads(reads), True)
    res = t.wait()
    same_segments(res, first)
    same_samples(res, first)                                                # an asynchronous ticket: the same bits as align_batch
    assert t.timing()["launches"] >= 1
    t.close()
    al.close()


# ---- 7. together with the border confidence ------------------------------------------------------------------------------------
def test_with_border_confidence_both_outputs_unchanged(models, sets):
    pore, band, reads = sets["rna002"]
    both, tm = run(models["syn5"], pore, band, reads, 16, W=8)
    assert tm["lp_inplace"] == 0 and tm["reads_strict"] == len(reads)      # k_read_queue<JOB_ALIGN | JOB_SAMPLE | JOB_BORDER, true>
    samples_only, _ = run(models["syn5"], pore, band, reads, 16)
    borders_only = run_off(models["syn5"], pore, band, reads, W=8)
    same_segments(both, borders_only)
    same_samples(both, samples_only)
    m = int(both.seg_offsets[-1])
    for c in ("border_probability", "border_window_probability"):
        assert np.array_equal(getattr(both, c)[:m].view(np.uint64), getattr(borders_only, c)[:m].view(np.uint64)), c


@pytest.mark.parametrize("name,layout", [("dna_r9", "separate"), ("rna002", "inplace"), ("dna_r9", "inplace")])
def test_with_border_confidence_the_other_launches(models, sets, want, monkeypatch, name, layout):
    """The three other launches that carry both phases: the separate layout's plain one, and the in-place layout's with the
    certified sweeps (rna002: every read carries the tie) and without. The paths against the yardstick as in the in-place case
    above, both outputs those of the launches that carry one phase, and the segments those of a launch that carries none."""
    pore, band, reads = sets[name]
    if layout == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    both, tm = run(models["syn5"], pore, band, reads, 16, W=8)
    samples_only, _ = run(models["syn5"], pore, band, reads, 16)
    borders_only = run_off(models["syn5"], pore, band, reads, W=8)
    off = run_off(models["syn5"], pore, band, reads)
    if layout == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
    assert tm["lp_inplace"] == (1 if layout == "inplace" else 0) and tm["launches"] == 1
    assert tm["reads_strict"] == (len(reads) if name == "rna002" else 0)
    check(both, want(members_of(sets, name), 16), 16, f"{name} {layout} behind the border phase")
    same_segments(both, off)
    same_segments(both, borders_only)
    same_samples(both, samples_only)
    m = int(both.seg_offsets[-1])
    for c in ("border_probability", "border_window_probability"):
        assert np.array_equal(getattr(both, c)[:m].view(np.uint64), getattr(borders_only, c)[:m].view(np.uint64)), c


# ---- 8. a failed read and a read of N = 2 --------------------------------------------------------------------------------------
def test_failed_read_and_two_column_read(models, sets, want):
    pore, band, reads = sets["dna_r9"]
    tiny = bcc.plain_reads(models["syn5"], "dna_r9", 31, 1, 5)[0]          # 5 bases at k = 5: N = 2, one output row
    failed = synth.SynthRead(reads[1].signal, reads[1].sequence[:40] + "N" + reads[1].sequence[41:])   # fails validation
    batch = [reads[0], failed, tiny, reads[2]]
    res, _ = run(models["syn5"], pore, band, batch, 16)
    assert res.status[1] != 0 and (res.status[[0, 2, 3]] == 0).all()
    assert res.n_segments[2] == 1 and (res.sample_dead == 0).all()
    a = int(res.seg_offsets[2])
    assert (res.sample_starts[:, a] == 0).all()                             # the one border there is: forced, row 0
    lo, hi = int(res.seg_offsets[1]), int(res.seg_offsets[2])
    assert (res.sample_starts[:, lo:hi] == 0).all()                         # rows of the failed read stay 0
    # reads 0 and 3 against the yardstick at THEIR index in this batch
    yard = want([("dna_r9", 0), ("dna_r9", 1), ("dna_r9", 1), ("dna_r9", 2)], 16)
    for i in (0, 3):
        starts, dead, undecided, _ = yard[i]
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        ok = ~undecided
        assert np.array_equal(res.sample_starts[ok, a:a + m], starts[ok]) and undecided.sum() <= 1, i


# ---- 9. the switch is per ticket and changes nothing else ----------------------------------------------------------------------
def test_switch_is_per_ticket_and_changes_nothing_else(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(7600 + j, 600, "rna004", mean, sd, (60, 120)) for j in range(2)]
    never = Aligner(models["syn9"], "rna004", device=0)                     # a handle that never switched it on
    base = [never.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads in data]
    never.close()
    al = Aligner(models["syn9"], "rna004", device=0)
    plan = [(0, 0), (4, 1), (16, 0), (0, 1), (4, 1)]                         # (K, data set), in submission order
    tickets = []
    for K, k in plan:
        al.set_posterior_samples(K, SEED)
        tickets.append(al.align_async(*synth.pack_reads(data[k]), True))
    al.set_posterior_samples(0)
    cap = int(base[0].cap) + int(base[1].cap)
    starts, dead = np.zeros((16, cap), dtype=np.uint32), np.zeros(600, dtype=np.uint32)
    out = _native.DynSampleOut(starts.ctypes.data_as(_native.c_u32_p), dead.ctypes.data_as(_native.c_u32_p), cap, 600, 16)
    results = []
    for (K, k), t in zip(plan, tickets):
        res = t.wait()
        results.append(res)
        same_segments(res, base[k])                                         # start, Z and probabilities: bit-equal to a plain run
        launches = t.timing()["launches"]
        if K == 0:
            assert res.sample_starts is None
            assert launches == 0                                            # published into the resident session (600 reads)
            with pytest.raises(ValueError, match="without dyn_aligner_set_posterior_samples"):
                t.fetch_samples(out)
        else:
            assert launches >= 1                                            # a launch of its own: no session, no merged launch
            assert res.sample_starts.shape[0] == K and (res.sample_dead == 0).all()
            m = int(res.seg_offsets[-1])
            for i in range(0, 600, 37):
                # every path is a segmentation: the first border is row 0 (forced), and a segment lasts two rows at least
                a, ns = int(res.seg_offsets[i]), int(res.n_segments[i])
                s = res.sample_starts[:, a:a + ns].astype(np.int64)
                assert (s[:, 0] == 0).all() and res.signal_positions[a] == 0 and (np.diff(s, axis=1) >= 2).all(), i
                assert s.max() <= len(data[k][i].signal) - 2
            out.count = 16
            t.fetch_samples(out)
            assert out.count == K and np.array_equal(starts[:K, :m], res.sample_starts[:, :m])
    same_samples(results[1], results[4])                                    # two tickets of the same reads, K and seed: the same bits
    for t in tickets:
        t.close()
    st = al.session_stats()
    assert st["sessions"] >= 1 and st["aborted"] == 0
    al.close()


def test_fetch_and_refusals(models, sets):
    pore, band, reads = sets["dna_r9"]
    sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
    al = Aligner(models["syn5"], pore, device=0)
    starts, dead = np.zeros((4, 4096), dtype=np.uint32), np.zeros(3, dtype=np.uint32)
    mk = lambda cap, n, cnt: _native.DynSampleOut(starts.ctypes.data_as(_native.c_u32_p), dead.ctypes.data_as(_native.c_u32_p), cap, n, cnt)  # noqa: E731
    with al.batch(sig, seq) as b:
        b.align(True)                          # switch off at submission
        al.set_posterior_samples(4, 1)
        with pytest.raises(ValueError, match="without dyn_aligner_set_posterior_samples"):
            b.fetch_samples(mk(4096, 3, 4))
        b.align(False)                         # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_samples(mk(4096, 3, 4))
        b.train()
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_samples(mk(4096, 3, 4))
        b.align(True)
        b.fetch_samples(mk(4096, 3, 4))
        for bad, word in ((mk(3, 3, 4), "capacity"), (mk(4096, 2, 4), "read count"), (mk(4096, 3, 3), "count")):
            with pytest.raises(ValueError, match=word):
                b.fetch_samples(bad)
        al.set_rescale(1)
        with pytest.raises(ValueError, match="dyn_aligner_set_rescale"):
            b.align(True)
        al.set_rescale(0)
        al.set_guide_rescue(4, 16)
        with pytest.raises(ValueError, match="dyn_aligner_set_guide_rescue"):
            b.align(True)
        al.set_guide_rescue(0, 0)
        al.set_auto_guide(16)
        with pytest.raises(ValueError, match="dyn_aligner_set_auto_guide"):
            al.align_async(*synth.pack_reads(reads), True)
        al.set_auto_guide(0)
    with pytest.raises(ValueError, match="carries a guide"):
        al.align_batch_auto(sig, seq, 16, 1)
    al.set_posterior_samples(0)
    al.set_band_retry(2)                       # not together with the band retry, whichever comes first
    with pytest.raises(ValueError, match="set_posterior_samples with set_band_retry"):
        al.set_posterior_samples(4)
    al.set_posterior_samples(0)                # (off is always accepted)
    al.set_band_retry(0)
    al.set_posterior_samples(4)
    with pytest.raises(ValueError, match="set_band_retry with set_posterior_samples"):
        al.set_band_retry(2)
    al.close()


# ---- 10. through the sink ---------------------------------------------------------------------------------------------------------
def test_through_the_sink(models, sets, tmp_path):
    pore, band, reads = sets["dna_r9"]
    al = Aligner(models["syn5"], pore, device=0)
    L = _native.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    flags = _native.DYN_CSV_BORDER_CONFIDENCE | _native.DYN_CSV_POSTERIOR_SAMPLES
    assert L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1,
                                  flags, C.byref(h), err, 1024) == 0, err.value
    sig, sig_off, seqs, seq_off = synth.pack_reads(reads)
    n = len(reads)
    rid = (C.c_char_p * n)(*[f"r{i}".encode() for i in range(n)])
    sid = (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)])
    starts = np.full(n, 100, dtype=np.int64)                                # the reads' aligned slices start at sample 100
    lengths = np.diff(np.asarray(sig_off).astype(np.int64)).astype(np.uint64)
    so = np.ascontiguousarray(seq_off, dtype=np.uint64)

    def submit(t):
        return L.dyn_csv_sink_submit(h, al._h, t._h, C.byref(t.result._c), n, seqs, so.ctypes.data_as(_native.c_u64_p), rid, sid,
                                     starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(_native.c_u64_p))

    al.set_border_confidence(8)
    lacking = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(lacking) == _native.DYN_ERR_INVALID_ARGUMENT and "DYN_CSV_POSTERIOR_SAMPLES" in al.last_error()
    al.set_posterior_samples(3, SEED)
    on = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(on) == 0
    assert L.dyn_csv_sink_wait(h, 1, -1) == 1
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    lines = zstd_io.decompress(open(tmp_path / "o.csv.zst", "rb").read()).split(b"\n")
    assert lines[0].endswith(b",polish,border_probability,border_window_probability,sample_starts")
    res = on.wait()
    assert len(lines) - 2 == int(res.n_segments.sum())
    for j in (0, 1, int(res.n_segments[0]) - 1):
        fields = lines[1 + j].split(b",")
        assert fields[-1] == ";".join(str(int(v) + 100) for v in res.sample_starts[:, j]).encode(), (j, lines[1 + j])
        assert int(fields[2]) == int(res.signal_positions[j]) + 100        # the `start` column: the same unit
    lacking.close()
    on.close()
    al.close()


# ---- 11. the device harness -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("psamp") / "libpsamp.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/posterior_samples.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.ps_run.restype = C.c_int
    return lib


P_SLOTS, CPL = 448, 7
HALF_LOG_2PI = float.fromhex("0x1.d67f1c864beb4p-1")
POISON = 0.0       # log-posterior 0: probability 1 -- a walk that read an out-of-band slot would take that way at once


def row_pos(s):
    lane, j = s // CPL, s % CPL
    return (j >> 1) * 128 + lane * 2 + (j & 1) if j < 6 else 384 + lane


class Lattice:
    """a read of T rows and N = 610 columns (slots wrap) with a narrow band, in all three layouts, built so that a walk has
    somewhere to go: random finite log-posteriors of a size at which a walk moves about as often as the band's diagonal does,
    -inf cells among them away from the band's edges (where a walk has but one way), a finite cell wherever the diagonal goes;
    every slot outside the band holds the poison. With dead_end, the lattice is cut: in front of the cut both ways on are -inf."""

    def __init__(self, seed=13, T=1900, N=610, bw=12, dead_end=False):
        rng = np.random.default_rng(seed)
        self.T, self.N, self.bw = T, N, bw
        self.ratio = N / T
        self.Zb, self.m1 = -1234.5678, 0.0
        self.rowmap = rng.permutation(T + 1).astype(np.uint32)
        B = 2 * bw + 3
        self.lp_in = np.full((T + 1, P_SLOTS, 2), POISON, dtype=np.float32)
        self.lp_wide = np.full((T, B, 2), POISON, dtype=np.float32)
        self.lpe_sep = np.full((T + 1, P_SLOTS), POISON, dtype=np.float32)
        self.bE = np.full((T + 1, P_SLOTS), -1000.0)
        # levels that hardly differ and samples near them: the LPM the separate layout rebuilds from two emissions (with m1 = 0)
        # stays within reach of the LPE beside it, so that a walk there moves about as often as the band's diagonal does
        mean, sd = rng.normal(0.0, 0.05, N - 1), rng.uniform(0.3, 0.6, N - 1)
        self.sig = rng.normal(0.0, 0.2, T - 1)
        self.par = np.stack([mean, 1.0 / sd, -np.log(sd), sd], axis=1).copy()
        self.inband = np.zeros((T + 2, N + 1), dtype=bool)
        self.lpm = np.full((T + 2, N + 1), -np.inf)      # float-valued: what the in-place and wide accessors return
        self.lpe = np.full((T + 2, N + 1), -np.inf)
        for t in range(1, T):
            start = int(t * self.ratio) - bw
            lo, hi = max(start, 1), min(start + 2 * bw + 1, N)
            self.inband[t, lo:hi] = True
            for n in range(lo, hi):
                inner = abs(n - int(t * self.ratio)) <= bw - 3     # -inf only away from the band's edges, where a walk has both ways
                vm = np.float32(-np.inf) if inner and rng.random() < 0.01 else np.float32(-rng.exponential(1.0) - 0.1)
                ve = np.float32(-np.inf) if inner and rng.random() < 0.003 else np.float32(-rng.exponential(0.5))
                self.lpm[t, n], self.lpe[t, n] = float(vm), float(ve)
        self.lpm[T - 1, :] = -np.inf                                        # an M cell of the last row has no way on
        # the corridor: E cells along the diagonal are finite, and so is the M cell that enters each column
        n = 0
        for t in range(1, T):
            want_n = min(int(t * self.ratio), N - 1)
            if want_n > n and t + 1 <= T - 1 and self.inband[t, n + 1]:
                n += 1
                self.lpm[t, n] = float(np.float32(-rng.exponential(1.0) - 0.1))
            elif self.inband[t, n]:
                self.lpe[t, n] = float(np.float32(-rng.exponential(0.5)))
        self.lpe[0, 0] = 0.0
        self.cut = None
        if dead_end:
            # three rows without a finite cell (a move skips a row, and the separate layout rebuilds LPM(t, .) from LPE(t-1, .)):
            # every sample arrives at a cell in front of them and finds both its ways -inf
            t = T // 2
            self.lpm[t + 1:t + 4, :] = -np.inf
            self.lpe[t + 1:t + 4, :] = -np.inf
            self.cut = t
        for t in range(1, T):
            start = int(t * self.ratio) - bw
            for n in range(max(start, 1), min(start + 2 * bw + 1, N)):
                pos = row_pos(n % P_SLOTS)
                self.lp_in[self.rowmap[t], pos] = (np.float32(self.lpm[t, n]), np.float32(self.lpe[t, n]))
                self.lp_wide[t, n - start + 1] = (np.float32(self.lpm[t, n]), np.float32(self.lpe[t, n]))
                self.lpe_sep[self.rowmap[t], pos] = np.float32(self.lpe[t, n])
                self.bE[self.rowmap[t], pos] = -np.inf if self.lpe[t, n] == -np.inf else -1000.0 - 0.01 * t + rng.uniform(-0.3, 0.3)

    def emis(self, x, n):
        mean, inv, nls, _ = self.par[n - 1]
        z = (x - mean) * inv
        return (z * z * -0.5 + nls) - HALF_LOG_2PI

    def separate_lpm(self):
        """BorderCellSeparate restated for every cell: LPM rebuilt from the float LPE and bE of (t-1, n-1), bE(t+1, n), two
        emissions, Zb and m1"""
        T, N, ib = self.T, self.N, self.inband
        out = np.full((T + 2, N + 1), -np.inf)
        for t in range(1, T - 1):
            for n in np.nonzero(ib[t, :N])[0].tolist():
                if not ib[t + 1, n]:
                    continue
                if t == 1:
                    if n != 1:
                        continue
                    fE_prev = 0.0
                else:
                    if not ib[t - 1, n - 1]:
                        continue
                    pos = row_pos((n - 1) % P_SLOTS)
                    l = self.lpe_sep[self.rowmap[t - 1], pos]
                    if l == -np.inf:
                        continue
                    fE_prev = (float(l) - self.bE[self.rowmap[t - 1], pos]) + self.Zb
                fM = (fE_prev + self.emis(self.sig[t - 1], n)) + self.m1
                bM = self.bE[self.rowmap[t + 1], row_pos(n % P_SLOTS)] + self.emis(self.sig[t], n)
                out[t, n] = (fM + bM) - self.Zb
        return out


@pytest.fixture(scope="module")
def lattices():
    return {False: Lattice(), True: Lattice(dead_end=True)}


@pytest.mark.parametrize("dead_end", [False, True])
@pytest.mark.parametrize("layout", [0, 1, 2])
def test_device_harness_walk(harness, lattices, layout, dead_end):
    """sample_kernels.hpp's three accessor pairs and the walk on a lattice of the test's own: 610 columns, a band of 25, every
    out-of-band slot poisoned with probability 1, -inf cells inside the band. Every path equals the host restatement over the
    values the accessors must return, entry for entry (a draw within 1e-14 p of its threshold, which the device's exp could turn,
    is counted, and there is at most one such path). With the lattice cut, every sample is dead: flagged 0xFFFFFFFF throughout,
    counted, and nothing beyond its own rows written."""
    la = lattices[dead_end]
    K, seed, read_index, cap, seg_off = 64, 77, 5, 700, 40
    with np.errstate(invalid="ignore", over="ignore"):
        lpm = la.separate_lpm() if layout == 0 else la.lpm
    # the lattice holds the device's own values: only the two exps can differ, by a few ulps
    starts, dead, undecided = psc.walk(lpm[:la.T, :la.N], la.lpe[:la.T, :la.N], seed, read_index, K, rel_margin=1e-14)
    FILL = 0xABCD1234
    out = np.full((K, cap), FILL, dtype=np.uint32)
    ndead = np.full(8, FILL, dtype=np.uint32)
    err = np.full(64, -1, dtype=np.int32)
    lp = (la.lpe_sep, la.lp_in, la.lp_wide)[layout]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = harness.ps_run(C.c_int(layout), C.c_int(la.T), C.c_int(la.N), C.c_int(la.bw), C.c_double(la.ratio), C.c_double(la.Zb),
                       C.c_double(la.m1), C.c_int(K), C.c_uint64(seed), C.c_uint32(read_index), C.c_uint64(cap), C.c_uint64(seg_off),
                       C.c_uint64(la.rowmap.size), p(la.rowmap), C.c_uint64(lp.size), p(lp), C.c_uint64(la.bE.size), p(la.bE),
                       C.c_uint64(la.sig.size), p(la.sig), C.c_uint64(la.par.shape[0]), p(la.par), p(out), p(ndead), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    got = out[:, seg_off:seg_off + la.N - 1]
    assert (out[:, :seg_off] == FILL).all() and (out[:, seg_off + la.N - 1:] == FILL).all()   # nothing outside the read's rows
    assert (ndead[np.arange(8) != read_index] == FILL).all()
    if dead_end:
        assert dead.all() and (got == psc.DEAD).all() and ndead[read_index] == K
        return
    assert not dead.any() and ndead[read_index] == 0
    differ = (got != starts).any(axis=1)
    print(f"layout {layout}: {int(undecided.sum())} undecided, {int(differ.sum())} differ")
    assert not (differ & ~undecided).any() and undecided.sum() <= 1
    assert len({row.tobytes() for row in got}) >= K // 2                    # the lanes draw their own numbers
