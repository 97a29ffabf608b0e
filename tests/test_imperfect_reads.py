"""align() on imperfect reads and near-duplicate tables, pinned by golden fixture G15 -- the CPU half.

G15 (tests/golden/g15_imperfect_reads.npz, written by tests/golden/make_golden_g15.py from the COMPILED REFERENCE; families in
tests/imperfect_families.py) holds the reference's borders, Z, status and message for reads whose basecall disagrees with the
signal, whose dwell is heavy-tailed, whose signal hugs or leaves the band, fits nothing or lies far outside every density, and
for reads on tables whose neighbouring k-mers lie 1e-6 .. 1e-16 apart -- where the traceback's exact comparison
(NT_aligner_api.cpp:445-448) has an on-path margin down to 0 between columns with DIFFERENT parameters. The tie rule flagged a
read only on bit-equal parameters when this fixture was first made; the plain arithmetic then left the reference's borders on 8
of 5 040 such reads (families "*_found": those reads, kept), and the rule now counts parameters within 1e-9 as tied.

Here: the generators moved into dynamont_amd.synth give what their originals gave; the oracle reproduces every G15 read bit for
bit; the CPU replay of the product's arithmetic in strict mode "ties" (tie_parity mode 8) lands on the reference's borders on
every near-duplicate read; the margin floors are what profiles/imperfect/decision_margins.json says; and an arithmetic that is
NOT the product's (the 4-operation emission of rounds 1-2) fails the near-duplicate families, i.e. they can fail.
The device half is tests/test_gpu_imperfect_reads.py.
"""
import json
import multiprocessing as mp
import os
import zlib

import numpy as np
import pytest

from conftest import ROOT, golden
from dynamont_amd import synth
from oracle import pyoracle
import imperfect_families as F
import tie_parity

WORKERS = min(16, os.cpu_count() or 1)
REPLAY_PER_IMPERFECT_FAMILY = 8


# ---- the generators are the ones they replace ------------------------------------------------------------------------------
def _variants_as_before(base, rng, sd_typ):
    """tests/test_gpu_train_chain.py's _variants as it stood before it moved to synth.stress_variants"""
    out = []
    for r in base:
        s = r.signal
        spiky = s.copy()
        spiky[rng.integers(0, len(s), size=len(s) // 37)] += 60 * sd_typ
        out.append(synth.SynthRead(spiky, r.sequence))
        far = s.copy()
        far[len(s) // 3] = 300.0
        far[len(s) // 2] = -5e3
        out.append(synth.SynthRead(far, r.sequence))
        out.append(synth.SynthRead(np.ascontiguousarray(s[rng.permutation(len(s))]), r.sequence))
        out.append(synth.SynthRead(np.ascontiguousarray(s[::-1]), r.sequence))
        flat = np.full(len(s), float(np.median(s)))
        out.append(synth.SynthRead(flat, r.sequence))
        cut = len(s) // 2
        squeezed = np.concatenate([s[:cut:5], np.repeat(s[cut:], 2)[: len(s) - len(s[:cut:5])]])
        out.append(synth.SynthRead(np.ascontiguousarray(squeezed), r.sequence))
        seq = list(r.sequence)
        called = seq[:9]
        for ch in seq[9:]:
            u = rng.random()
            if u < 0.015:
                continue
            if u < 0.03:
                called.append("ACGT"[rng.integers(0, 4)])
            called.append("ACGT"[rng.integers(0, 4)] if rng.random() < 0.05 else ch)
        out.append(synth.SynthRead(s.copy(), "".join(called)))
    return out


def _crc(reads):
    c = 0
    for r in reads:
        c = zlib.crc32(r.sequence.encode(), zlib.crc32(r.signal.tobytes(), c))
    return c


@pytest.mark.parametrize("pore,nb,crc", [("rna004", (250, 420), 1092939408), ("dna_r9", (150, 400), 3344318386), ("rna002", (100, 300), 2833815843)])
def test_stress_variants_are_the_train_tests_variants(models, pore, nb, crc):
    """seed 950, the reads of test_train_posterior_chain_under_stress: array_equal to the function as it stood, and to the
    checksum taken from it before the move"""
    from conftest import model_for
    import test_gpu_train_chain
    _, mean, sd = synth.read_model_file(model_for(models, pore))
    base = synth.make_reads(77, 5, pore, mean, sd, nb)
    old = _variants_as_before(base, np.random.default_rng(950), float(np.median(sd)))
    new = test_gpu_train_chain._variants(base, np.random.default_rng(950), float(np.median(sd)))
    assert len(old) == len(new) == 35
    for a, b in zip(old, new):
        assert np.array_equal(a.signal, b.signal) and a.sequence == b.sequence
    assert _crc(new) == crc


def test_imperfect_read_is_the_tools_generator_and_dna_reads_have_no_pad(models):
    """RNA: the reads tools/realistic_train_reads.py made before its generator moved (checksums taken from it, seed 31337).
    DNA: the same draws without the polyA pad -- no read starts with nine A's by construction."""
    _, mean, sd = synth.read_model_file(models["syn9"])
    mean_c, sd_c = synth.code_order_table(mean, sd, 9, True)
    for heavy, crc in ((False, 2647001773), (True, 2072390736)):
        rng = np.random.default_rng(31337)
        reads = [synth.imperfect_read(rng, mean_c, sd_c, 9, 300, heavy, 0.05, 0.03, True) for _ in range(4)]
        assert _crc(reads) == crc and all(r.sequence.startswith("A" * 9) for r in reads)
    rng = np.random.default_rng(31337)
    dna = [synth.imperfect_read(rng, mean, sd, 9, 300, True, 0.05, 0.03, False) for _ in range(32)]
    assert not any(r.sequence.startswith("A" * 9) for r in dna)
    assert all(len(r.signal) >= 2 * (len(r.sequence) - 8) for r in dna)


@pytest.mark.parametrize("k,flavour", [(5, "mean"), (5, "stdev"), (9, "mean")])
def test_near_duplicate_table_puts_neighbouring_kmers_into_one_cluster(k, flavour):
    """a quarter of the neighbouring columns of a random read carry DISTINCT k-mers of one cluster, their parameters
    differing by about 10^-e and, for e <= 14, never bit-equal"""
    mean, sd = synth.near_duplicate_table(k, range(9, 15), 11, flavour, 0.2)
    moved, other = (mean, sd) if flavour == "mean" else (sd, mean)
    rng = np.random.default_rng(5)
    digits = rng.integers(0, 4, size=4000)
    codes = synth._seq_codes(digits, k)
    a, b = codes[:-1], codes[1:]
    same_cluster = (other[a] == other[b]) if flavour == "stdev" else (np.abs(mean[a] - mean[b]) < 1e-8)
    distinct = a != b
    near = same_cluster & distinct
    assert 0.15 < near.mean() < 0.35
    gap = np.abs(moved[a[near]] - moved[b[near]])
    assert (gap > 0).all() and gap.max() < 5e-9 and np.median(gap) < 1e-9
    if flavour == "mean":
        assert np.array_equal(sd, np.full(4 ** k, 0.2))
    # a k-mer and its reverse share their composition, hence their cluster: the RNA pores' reversed storage keeps the clusters
    m_rna, s_rna = synth.code_order_table(mean, sd, k, True)
    assert np.array_equal(s_rna, sd) if flavour == "mean" else np.array_equal(m_rna, mean)
    assert np.abs((m_rna if flavour == "mean" else s_rna) - moved).max() < 5e-9


# ---- G15 ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g15(tmp_path_factory, oracle_built):
    g = golden("g15_imperfect_reads.npz")
    assert json.loads(str(g["families"])) == list(F.FAMILIES)
    tables = F.write_tables(str(tmp_path_factory.mktemp("g15models")))
    fams = {}
    for name, fam in F.FAMILIES.items():
        reads = F.reads_of(name, tables)
        assert np.array_equal(np.array([len(r.signal) for r in reads], dtype=np.int32), g[name + "_S"]), f"{name}: regenerated inputs differ"
        assert np.array_equal(np.array([F.signal_crc(r) for r in reads], dtype=np.uint32), g[name + "_crc"]), f"{name}: regenerated inputs differ"
        fams[name] = dict(fam=fam, model=tables[fam.table][0], reads=reads)
    return g, fams


def want_of(g, name, i):
    """the reference's answer to read i of a family: None where it refused the read"""
    if g[name + "_status"][i]:
        return None
    a, b = int(g[name + "_seg_off"][i]), int(g[name + "_seg_off"][i + 1])
    return dict(signal_positions=g[name + "_sigpos"][a:b].astype(np.uint64), sequence_positions=g[name + "_seqpos"][a:b].astype(np.uint64),
                Z=float(g[name + "_Z"][i]), all_M=bool(g[name + "_all_M"][i]))


def test_g15_holds_what_the_issue_asks_for(g15):
    g, fams = g15
    for pore in F.PORES:
        names = [n for n, f in fams.items() if f["fam"].pore == pore and f["fam"].band == 400 and f["fam"].kind in ("errors", "variant", "edge")]
        assert len(names) == 6 + 7 + 1
        assert sum(f["fam"].band == 50 for f in fams.values() if f["fam"].pore == pore) == 2
    for name, f in fams.items():
        fam, n = f["fam"], len(f["reads"])
        assert n >= {"near": 120, "cfg2": 32, "found": 2}.get(fam.kind, 16)
        assert g[name + "_status"].mean() <= 0.10, name             # refused by the reference: recorded, and rare
        assert g[name + "_sigpos"].dtype == np.int32 and g[name + "_seqpos"].dtype == np.int32
        if fam.band == 600:   # half band min(300, columns / 2) > 223: the generic wide-band kernel
            k = synth.PORES[fam.pore][2]
            assert min((len(r.sequence) - k + 2) // 2 for r in f["reads"]) > 223
        if fam.kind == "cfg2":
            assert min(len(r.signal) for r in f["reads"]) > 15000
    refused = {n: [str(m) for m in g[n + "_message"] if str(m)] for n in fams if g[n + "_status"].any()}
    assert refused and all(set(v) == {"Alignment failed: alignment scores do not match"} for v in refused.values())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g15_imperfect_reads.npz")) <= 1000000


_W = {}


def _orc_init(model, pore_id, band):
    _W["orc"] = pyoracle.Oracle(model, pore_id, band)


def _orc_one(job):
    try:
        r = _W["orc"].align(job[0], job[1], True)
    except RuntimeError as e:
        return str(e)
    return (r["signal_positions"], r["sequence_positions"], r["Z"], all(s == "M" for s in r["states"]),
            _W["orc"].last_decision_margin_distinct(), _W["orc"].last_decision_margin_distinct_params())


def test_oracle_reproduces_g15_bit_for_bit(g15):
    """every read of every family: borders, Z bits, the all-M states, the refusal and its message, both margins"""
    g, fams = g15
    for name, f in fams.items():
        fam = f["fam"]
        with mp.get_context("fork").Pool(WORKERS, initializer=_orc_init, initargs=(f["model"], synth.PORES[fam.pore][0], fam.band)) as pool:
            got = pool.map(_orc_one, [(r.signal, r.sequence) for r in f["reads"]], chunksize=2)
        for i, r in enumerate(got):
            want = want_of(g, name, i)
            if want is None:
                assert r == str(g[name + "_message"][i]), (name, i, r)
                continue
            assert not isinstance(r, str), (name, i, r)
            assert np.array_equal(r[0], want["signal_positions"]) and np.array_equal(r[1], want["sequence_positions"]), (name, i)
            assert r[2] == want["Z"] and r[3] == want["all_M"], (name, i)
            assert r[4] == g[name + "_margin_kmer"][i] and r[5] == g[name + "_margin_params"][i], (name, i)


@pytest.fixture(scope="module")
def replay_so(tmp_path_factory):
    return tie_parity.build_replay(str(tmp_path_factory.mktemp("replay")))


def _rp_init(so, model, pore_id, band, mode):
    _W["rp"] = tie_parity.Replay(so, model, pore_id, band, mode=mode)


def _rp_one(job):
    sig, seq, rows = job
    _W["rp"].set_strict_rows(rows)
    try:
        r = _W["rp"].align(sig, seq, True)
    except RuntimeError as e:
        return str(e)
    return r["signal_positions"], r["sequence_positions"], r["Z"]


def _replay(so, f, picks, rows, mode):
    fam = f["fam"]
    with mp.get_context("fork").Pool(WORKERS, initializer=_rp_init, initargs=(so, f["model"], synth.PORES[fam.pore][0], fam.band, mode)) as pool:
        return pool.map(_rp_one, [(f["reads"][i].signal, f["reads"][i].sequence, int(rows[i])) for i in picks], chunksize=2)


def _tie_rows(f):
    from dynamont_amd import Aligner
    fam, reads = f["fam"], f["reads"]
    al = Aligner(f["model"], fam.pore, band=fam.band, device="host")
    _, _, kms = al.validate([len(r.signal) for r in reads], [r.sequence for r in reads])
    rows = [al.tie_rows(kms[i], len(reads[i].signal)) for i in range(len(reads))]
    al.close()
    return rows


def test_replay_of_mode_ties_gives_the_references_borders(g15, replay_so):
    """CPU: the product's arithmetic exactly where the kernels use it -- certified backward sweep and certified forward blocks up
    to dyn_tie_rows on flagged reads, the plain table softplus everywhere else (tie_parity mode 8) -- on EVERY near-duplicate
    read and on the first 8 reads of every other family: the reference's borders; the reference's Z bits on every flagged read;
    1e-9 relative on the others; a read the reference refuses is refused. dyn_tie_rows itself is what the fixture recorded.
    (Under the rule of bit-equal parameters the eight reads of rna004_near9_mean_12_16_found and rna004_near9_stdev_9_15_found
    came out off the reference's borders here: test_the_old_rule_fails_the_found_reads.)"""
    g, fams = g15
    widened = refused_seen = 0
    for name, f in fams.items():
        fam = f["fam"]
        rows = _tie_rows(f)
        assert np.array_equal(np.array(rows, dtype=np.uint32), g[name + "_rows"]), name
        picks = list(range(len(f["reads"]) if fam.kind in ("near", "found") else REPLAY_PER_IMPERFECT_FAMILY))
        picks += [i for i in np.flatnonzero(g[name + "_status"]).tolist() if i not in picks]   # and every read the reference refuses
        got = _replay(replay_so, f, picks, rows, 8)
        for i, r in zip(picks, got):
            want = want_of(g, name, i)
            if want is None:
                assert r == str(g[name + "_message"][i]), (name, i, r)
                refused_seen += 1
                continue
            assert not isinstance(r, str), (name, i, r)
            assert np.array_equal(r[0], want["signal_positions"]) and np.array_equal(r[1], want["sequence_positions"]), (name, i, rows[i])
            if rows[i]:
                assert r[2] == want["Z"], (name, i)
                widened += not g[name + "_bit_equal_tie"][i] and g[name + "_margin_params"][i] < 1e-12
            else:
                assert abs(r[2] - want["Z"]) <= 1e-9 * max(1.0, abs(want["Z"])), (name, i)
    assert refused_seen >= 3   # the 2e5 read of the edge families
    assert widened >= 20   # reads with a margin in the noise between columns that are NOT bit-equal: flagged by the widened rule only


def test_the_old_rule_fails_the_found_reads(g15, replay_so):
    """What the widened rule is for: with the rule of BIT-EQUAL parameters (strict rows only where the fixture's bit_equal_tie
    says so; none of the found reads has such a pair) the replay of mode "ties" leaves the reference's borders on every read of
    the two families the campaign found deviating."""
    g, fams = g15
    for name in ("rna004_near9_mean_12_16_found", "rna004_near9_stdev_9_15_found"):
        f = fams[name]
        assert not g[name + "_bit_equal_tie"].any() and (g[name + "_rows"] != 0).all()
        got = _replay(replay_so, f, list(range(len(f["reads"]))), [0] * len(f["reads"]), 8)
        for i, r in enumerate(got):
            want = want_of(g, name, i)
            assert not (np.array_equal(r[0], want["signal_positions"]) and np.array_equal(r[1], want["sequence_positions"])), (name, i)


def test_margin_floors_and_the_tie_rule_are_what_the_record_says(g15):
    """The margin statement, from the fixture instead of hearsay: per family the floor of the parameter-distinct margin equals
    profiles/imperfect/decision_margins.json. Ordinary tables: the floor is >= 1e-7 on every imperfect family (test_g13's bar)
    and the rule flags exactly the reads with bit-equal neighbours, as it always did. Near-duplicate tables: reads whose
    neighbouring columns are NOT bit-equal and whose margin is below 1e-12 EXIST in every table with gaps of 1e-12 or less (no
    margin argument covers them: the rule must flag them, and does); what the rule leaves unflagged keeps a margin >= 1e-9;
    and 1e-9 is the smallest decade of the recorded sweep for which that holds -- the threshold comes from the reference's
    margins, not from what the kernels get right."""
    g, fams = g15
    rec_all = json.load(open(os.path.join(ROOT, "profiles", "imperfect", "decision_margins.json")))
    rec = rec_all["families"]
    assert list(rec) == list(fams)
    for name, f in fams.items():
        ok = g[name + "_status"] == 0
        mpar, rows, bit_equal = g[name + "_margin_params"], g[name + "_rows"], g[name + "_bit_equal_tie"]
        unflagged = ok & (rows == 0)
        assert rec[name]["refused"] == int((~ok).sum()) and rec[name]["flagged"] == int((rows != 0).sum())
        assert rec[name]["flagged_by_bit_equal_parameters"] == int(bit_equal.sum())
        assert rec[name]["distinct_parameter_decisions"]["min"] == float(mpar[ok].min()), name
        assert rec[name]["unflagged"]["reads"] == int(unflagged.sum())
        assert rec[name]["unflagged"]["reads_below_1e-9"] == int((mpar[unflagged] < 1e-9).sum()), name
        if f["fam"].kind not in ("near", "found"):
            assert mpar[ok].min() >= 1e-7, (name, float(mpar[ok].min()))
            assert (g[name + "_margin_kmer"][ok] >= 1e-7).all(), name
            assert np.array_equal(rows != 0, bit_equal), name          # ordinary tables: the rule costs what it cost
            continue
        assert not (bit_equal & (rows == 0)).any(), name
        assert (mpar[unflagged] >= 1e-9).all(), name
        if f["fam"].kind == "near" and ("12_16" in name or "stdev" in name):
            assert int((ok & ~bit_equal & (mpar < 1e-12)).sum()) >= 5, name
        elif f["fam"].kind == "near":
            assert int((ok & ~bit_equal & (mpar < 1e-9)).sum()) >= 5, name
    sweep = rec_all["tie_rule_sweep"]
    assert sweep["chosen_tau"] == "1e-9" and F.TIE_TAU == 1e-9
    below = {s["tau"]: s["unflagged_below_1e-9"] for s in sweep["sweep"]}
    assert below["1e-9"] == 0 and below["1e-10"] > 0 and all(below[f"1e-{e}"] > 0 for e in range(10, 17))


def test_the_near_duplicate_families_can_fail(g15, replay_so):
    """Mutation check: the 4-operation emission of rounds 1-2 (constants pre-added, one FMA: tie_parity mode 2), an arithmetic a
    few ulp from the product's, leaves the reference's borders on near-duplicate reads the product's replay gets right
    (measured: 5 of the 720 reads -- dna_r9_near5_mean_12_16 read 95, dna_r9_near5_stdev_9_15 read 58, rna004_near9_mean_12_16
    reads 50, 51, 111), every one of them a read whose margin is below 1e-9. A fixture no arithmetic change can fail would pin nothing."""
    g, fams = g15
    off = []
    for name in F.NEAR_FAMILIES:
        f = fams[name]
        picks = list(range(len(f["reads"])))
        got = _replay(replay_so, f, picks, [0] * len(picks), 2)
        for i, r in zip(picks, got):
            want = want_of(g, name, i)
            if isinstance(r, str) or not (np.array_equal(r[0], want["signal_positions"]) and np.array_equal(r[1], want["sequence_positions"])):
                off.append((name, i))
    print("mode 2 leaves the reference's borders on", off)
    assert len(off) >= 1
    for name, i in off:
        assert g[name + "_margin_params"][i] < 1e-9, (name, i)
