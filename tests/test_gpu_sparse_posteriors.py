"""GPU (-m gpu): the forward sweep stores a lane group's float LPE only where exp() of it does not underflow
(dynamont_amd/csrc/lpe_liveness.hpp). Every case runs the same reads through
  * a handle as created (floor -750),
  * a handle created under DYN_LPE_STORE_FLOOR=dense (every cell stored: the control),
  * the CPU oracle, Oracle.align(calc=True).
Status, Z and every integer column are equal in all three; the probabilities of the two handles are bit-equal, and within 1e-6
of the oracle's (tests/test_gpu_parity.py's PROB_TIGHT). One more run under DYN_LPE_STORE_FLOOR=-5 puts path cells themselves
below the floor: those posteriors, and only those, become exactly 0.0."""
import json
import math

import numpy as np
import pytest

from conftest import golden, model_for
from dynamont_amd import Aligner, synth
from oracle.pyoracle import Oracle
import imperfect_families as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib", "oracle_built")]

PROB_TIGHT = 1e-6   # tests/test_gpu_parity.py


def handle(monkeypatch, floor, model, pore, **kw):
    """a handle created under DYN_LPE_STORE_FLOOR=floor (None: as created); the switch is read once, at creation"""
    if floor is None:
        monkeypatch.delenv("DYN_LPE_STORE_FLOOR", raising=False)
    else:
        monkeypatch.setenv("DYN_LPE_STORE_FLOOR", floor)
    al = Aligner(model, pore, device=0, **kw)
    monkeypatch.delenv("DYN_LPE_STORE_FLOOR", raising=False)
    return al


def assert_same_bits(a, b, what):
    """two batch results: status, Z, every integer column and every probability bit for bit"""
    assert np.array_equal(a.status, b.status), what
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64)), what
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets), what
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "states"):
        assert np.array_equal(getattr(a, col)[:m], getattr(b, col)[:m]), (what, col)
    assert np.array_equal(a.probabilities[:m], b.probabilities[:m], equal_nan=True), what
    assert np.array_equal(a.probabilities[:m].view(np.uint64), b.probabilities[:m].view(np.uint64)), what


def assert_oracle(res, orc, reads, what, expect_refused=None):
    """every read against Oracle.align(calc=True): its message when it refuses, else integer columns equal, |dp| <= 1e-6"""
    worst, refused = 0.0, 0
    for i, r in enumerate(reads):
        try:
            want = orc.align(r.signal, r.sequence, True)
        except RuntimeError as e:
            assert res.status[i] != 0 and res.error(i) == str(e), (what, i, res.error(i), str(e))
            refused += 1
            continue
        got = res.read(i)
        assert np.array_equal(got["sequence_positions"], want["sequence_positions"]), (what, i)
        assert np.array_equal(got["signal_positions"], want["signal_positions"]), (what, i)
        assert got["states"] == want["states"], (what, i)
        assert abs(got["Z"] - want["Z"]) <= 1e-9 * max(1.0, abs(want["Z"])), (what, i)
        dp = float(np.abs(got["probabilities"] - want["probabilities"]).max())
        worst = max(worst, dp)
        assert dp <= PROB_TIGHT, (what, i, dp)
    print(f"{what}: {len(reads)} reads, {refused} refused by the oracle, max |dp| against the oracle {worst:.2e}")
    if expect_refused is not None:
        assert (refused > 0) == expect_refused, (what, refused)
    return refused


def three_way(monkeypatch, model, pore, reads, what, band=400, expect_refused=None, prepare=None, **kw):
    sigs, seqs = [r.signal for r in reads], [r.sequence for r in reads]
    out = []
    for floor in (None, "dense"):
        al = handle(monkeypatch, floor, model, pore, band=band, **kw)
        if prepare:
            prepare(al)
        out.append(al.align_batch(sigs, seqs, True))
        al.close()
    default, dense = out
    assert_same_bits(default, dense, what)
    assert_oracle(default, Oracle(model, synth.PORES[pore][0], band), reads, what, expect_refused)
    return default, dense


def reads_for(models, pore, seed, n, bases, **kw):
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    return synth.make_reads(seed, n, pore, mean, sd, bases, **kw)


@pytest.fixture(scope="module")
def long_rna004(models):
    """500-900 bases: more than 448 lattice columns, so the slot ring wraps, the path crosses every lane-group border and the
    traceback walks many 64-row blocks"""
    return reads_for(models, "rna004", 6101, 16, (500, 900))


def test_long_reads_ring_wraps(models, monkeypatch, long_rna004):
    default, _ = three_way(monkeypatch, models["syn9"], "rna004", long_rna004, "rna004 500-900 bases", expect_refused=False)
    assert (default.status == 0).all() and int(default.n_segments.max()) > 448


def test_short_reads_band_narrower_than_the_slots(models, monkeypatch):
    """bw = N / 2: most lanes of a row lie outside the band (their LPE is -inf, their groups are never stored)"""
    three_way(monkeypatch, models["syn9"], "rna004", reads_for(models, "rna004", 6102, 24, (30, 300)), "rna004 30-300 bases")
    three_way(monkeypatch, models["syn5"], "rna002", reads_for(models, "rna002", 6103, 16, (30, 300)), "rna002 30-300 bases")


@pytest.mark.parametrize("band", [7, 31, 60])
def test_narrow_bands(models, monkeypatch, band):
    three_way(monkeypatch, models["syn5"], "dna_r9", reads_for(models, "dna_r9", 6104 + band, 16, (40, 400)), f"dna_r9 band {band}",
              band=band)


def test_stress_variants(models, monkeypatch):
    """flat, permuted, reversed, squeezed, spiky, far-out, mis-called: diffuse posteriors (several live groups per row, rows
    whose cells all lie far below 0) and reads both sides refuse"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    base = synth.make_reads(6105, 3, "rna004", mean, sd, (150, 520))
    reads = synth.stress_variants(base, np.random.default_rng(6106), float(np.median(sd)))
    assert len(reads) == 7 * len(base)
    three_way(monkeypatch, models["syn9"], "rna004", reads, "rna004 stress variants")


def test_imperfect_reads_of_g15(monkeypatch, tmp_path_factory):
    """reads with substitutions and indels in the basecall, the inputs of golden fixture G15 (regenerated, checked by CRC)"""
    g = golden("g15_imperfect_reads.npz")
    assert json.loads(str(g["families"])) == list(F.FAMILIES)
    name = "rna004_heavy_10_6_band50"
    fam = F.FAMILIES[name]
    tables = F.write_tables(str(tmp_path_factory.mktemp("g15models")), [fam.table])
    reads = F.reads_of(name, tables)
    assert np.array_equal(np.array([F.signal_crc(r) for r in reads], dtype=np.uint32), g[name + "_crc"])
    three_way(monkeypatch, tables[fam.table][0], fam.pore, reads[:16], name, band=fam.band)
    name = next(n for n, f in F.FAMILIES.items() if f.pore == "rna004" and f.kind == "errors" and f.band == 400 and f.arg[0])
    fam = F.FAMILIES[name]
    reads = F.reads_of(name, tables)
    assert np.array_equal(np.array([F.signal_crc(r) for r in reads], dtype=np.uint32), g[name + "_crc"])
    three_way(monkeypatch, tables[fam.table][0], fam.pore, reads[:16], name, band=fam.band)


def test_polya_reads_take_the_certified_sweeps(models, monkeypatch):
    """cfg2_polya-style reads in the default strict mode `ties`: every read is flagged, the STRICT instantiation stores"""
    reads = reads_for(models, "rna004", 6107, 16, (150, 500), polya=(20, 150))
    sigs, seqs = [r.signal for r in reads], [r.sequence for r in reads]
    al = handle(monkeypatch, None, models["syn9"], "rna004")
    with al.batch(sigs, seqs) as b:
        b.align(True)
        assert b.timing()["reads_strict"] == len(reads)
    al.close()
    three_way(monkeypatch, models["syn9"], "rna004", reads, "rna004 poly-A, mode ties", expect_refused=False)


def test_page_starved_pool_reuses_pages_between_reads(models, monkeypatch):
    """tests/test_gpu_parity.py's page-starved launch at its smallest parameters (8 workgroups, 0.3 of the pages the waves in
    flight want), separate layout: a wave's pages come from the free list, so the floats a row does not store are other reads'"""
    reads = reads_for(models, "rna004", 6108, 64, (100, 700))
    lens = sorted((len(r.signal) for r in reads), reverse=True)
    row = 448 * 12 + 64
    budget = int(max(0.3 * sum(lens[:32]) * row, 1.3 * lens[0] * row))
    monkeypatch.setenv("DYN_FORCE_LAYOUT", "separate")
    monkeypatch.setenv("DYN_QUEUE_CUS", "8")
    al = handle(monkeypatch, None, models["syn9"], "rna004")
    want = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
    al.close()
    default, _ = three_way(monkeypatch, models["syn9"], "rna004", reads, "page-starved launch", prepare=lambda al: al.set_mem_budget(budget))
    assert_same_bits(default, want, "page-starved against the unconstrained pool")


def test_resident_session_equals_dense(models, monkeypatch):
    """the resident read queue (k_session, the benchmark's kernel): one ticket of 640 reads, default against dense bit for
    bit; the oracle on its first 12 reads (the other cases cover the oracle; 640 reads of it would take a minute)"""
    reads = reads_for(models, "rna004", 6109, 640, (100, 420))
    packed = synth.pack_reads(reads)
    out = []
    for floor in (None, "dense"):
        al = handle(monkeypatch, floor, models["syn9"], "rna004")
        t = al.align_async(*packed, True)
        out.append(t.wait())
        assert t.timing()["launches"] == 0          # published into the resident session
        t.close()
        al.close()
    assert_same_bits(out[0], out[1], "resident session")
    assert_oracle(out[0], Oracle(models["syn9"], synth.PORES["rna004"][0]), reads[:12], "resident session, first reads")


def test_border_confidence_and_band_margin_switch_to_dense(models, monkeypatch):
    """the border-confidence phase reads whole windows of LPE: its launch stores every cell, whatever the floor -- the two
    columns of a handle as created equal those of a dense handle and of a handle whose floor would drop path cells; the band
    margins (computed from the borders) and the segments come out as without the switches"""
    reads = reads_for(models, "rna004", 6110, 16, (150, 600))
    sigs, seqs = [r.signal for r in reads], [r.sequence for r in reads]
    res = {}
    for floor in (None, "dense", "-5"):
        al = handle(monkeypatch, floor, models["syn9"], "rna004")
        al.set_border_confidence(8)
        al.set_band_margin(True)
        res[floor] = al.align_batch(sigs, seqs, True)
        al.close()
    al = handle(monkeypatch, "dense", models["syn9"], "rna004")
    plain = al.align_batch(sigs, seqs, True)
    al.close()
    for floor in (None, "-5"):
        for col in ("border_probability", "border_window_probability", "band_margin_low", "band_margin_high", "band_edge_rows"):
            a, b = getattr(res[floor], col), getattr(res["dense"], col)
            assert a is not None and np.asarray(a).tobytes() == np.asarray(b).tobytes(), (floor, col)
        assert_same_bits(res[floor], res["dense"], f"border confidence on, floor {floor}")
    assert_same_bits(res[None], plain, "switches on against switches off")
    assert float(res[None].border_window_probability[:int(res[None].seg_offsets[-1])].max()) > 0.5   # (the columns are filled)


def test_dead_path_cells_become_exact_zeros(models, monkeypatch, long_rna004):
    """DYN_LPE_STORE_FLOOR=-5 puts path cells below the floor. Borders equal dense; a probability is bit-equal to dense or
    exactly 0.0, and 0.0 only where the dense value lies below exp(-5) (1 + 1e-3) (the float rounding of LPE is far inside
    the 1e-3); at least one 0.0 occurs; the CPU's count of posteriors below exp(-5) bounds their number. The long rna004
    reads and one homopolymer read (see below; the oracle needs 6 s for it)."""
    # Reads that fit their basecall never get there: a path cell's own lane group always holds a posterior above exp(-5)
    # (measured: 0 zeros in the 11 115 segments of the long reads, 0 in 14 991 with 14 stress variants added). A path cell
    # below exp(-5) needs the row's mass spread over more than 150 columns: a homopolymer (every column the same k-mer, every
    # monotone path as likely as the next) whose spread, growing with the square root of its length, reaches that at about
    # 100 k samples. 120 000 samples over 36 000 bases: the oracle's medians are 0.0056 .. 0.02, 20 286 below exp(-5).
    # Measured on the GPU: 20 286 of the batch's 47 228 probabilities become 0.0, the largest dense value among them 6.738e-03.
    kmers, mean, sd = synth.read_model_file(models["syn9"])
    a9 = kmers.index("A" * 9)
    homopolymer = synth.SynthRead(mean[a9] + sd[a9] * np.random.default_rng(6113).standard_normal(120000), "A" * 36008)
    reads = list(long_rna004) + [homopolymer]
    sigs, seqs = [r.signal for r in reads], [r.sequence for r in reads]
    out = {}
    for floor in ("dense", "-5"):
        al = handle(monkeypatch, floor, models["syn9"], "rna004")
        out[floor] = al.align_batch(sigs, seqs, True)
        al.close()
    dense, low = out["dense"], out["-5"]
    assert np.array_equal(dense.status, low.status) and (dense.status == 0).all()
    assert np.array_equal(dense.Z.view(np.uint64), low.Z.view(np.uint64))
    assert np.array_equal(dense.n_segments, low.n_segments) and np.array_equal(dense.seg_offsets, low.seg_offsets)
    m = int(dense.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "states"):
        assert np.array_equal(getattr(dense, col)[:m], getattr(low, col)[:m]), col
    pd, pl = dense.probabilities[:m], low.probabilities[:m]
    same = pd.view(np.uint64) == pl.view(np.uint64)
    zero = ~same & (pl.view(np.uint64) == 0)
    assert (same | zero).all(), "a probability is neither dense's nor +0.0"
    n_zero = int(zero.sum())
    print(f"floor -5: {n_zero} of {m} probabilities became 0.0; largest dense value among them {pd[zero].max() if n_zero else 0.0:.3e}")
    assert n_zero >= 1
    assert (pd[zero] < math.exp(-5.0) * (1.0 + 1e-3)).all()
    orc = Oracle(models["syn9"], synth.PORES["rna004"][0])
    below = sum(int((orc.align(r.signal, r.sequence, True)["probabilities"] < math.exp(-5.0)).sum()) for r in reads)
    assert n_zero <= below, (n_zero, below)
