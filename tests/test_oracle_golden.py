"""CPU: the oracle (oracle/nt_oracle.c) against every golden vector generated from the compiled
reference (tests/golden/make_golden.py). Bit-exact on everything: same libm, same op order."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, model_for
from dynamont_amd import synth
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("oracle_built")


def exact(res, g, p):
    assert res["Z"] == float(g[p + "Z"])
    assert np.array_equal(res["sequence_positions"], g[p + "seqpos"].astype(np.uint64))
    assert np.array_equal(res["signal_positions"], g[p + "sigpos"].astype(np.uint64))
    assert np.array_equal(res["probabilities"], g[p + "prob"])
    assert all(s == "M" for s in res["states"])


def test_g1_cfg1(models, tmp_path):
    g = golden("g1_cfg1.npz")
    # the real rna002 5-mer values are stored in the fixture (file order): rebuild the TSV
    real = tmp_path / "rna002_5mer.model"
    names = synth.kmer_strings(5)
    with open(real, "w") as w:
        w.write("kmer\tlevel_mean\tlevel_stdv\n")
        for n, m, s in zip(names, g["real_model_mean"], g["real_model_stdev"]):
            w.write(f"{n}\t{float(m)!r}\t{float(s)!r}\n")
    for tag, path in (("real_", str(real)), ("syn_", models["syn5"])):
        res = Oracle(path, 0).align(g[tag + "signal"], str(g[tag + "sequence"]), True)
        exact(res, g, tag)
    # the first segment starts at sample 0 and there are Kc segments
    assert int(g["syn_sigpos"][0]) == 0 and len(g["syn_sigpos"]) == len(str(g["syn_sequence"])) - 4


def test_g2_rna004_inputs_regenerate_and_match(models):
    g = golden("g2_rna004.npz")
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(int(g["seed"]), int(g["n_reads"]), "rna004", mean, sd, (200, 2000))
    orc = Oracle(models["syn9"], 1)
    for i, rd in enumerate(reads):
        assert hashlib.sha256(rd.signal.tobytes()).hexdigest() == str(g[f"r{i}_sha"])
        if len(rd.signal) > 9000 and i % 2:  # keep the CPU suite in minutes: every long read is still
            continue                        # covered on the GPU side against the same fixture
        exact(orc.align(rd.signal, rd.sequence, True), g, f"r{i}_")


def test_g3_short_reads_and_bands(models):
    g = golden("g3_short.npz")
    cache = {}
    for i in range(int(g["n_cases"])):
        p = f"c{i}_"
        pore = str(g[p + "pore"])
        band = int(g[p + "band"]) if p + "band" in g else 400
        key = (pore, band)
        if key not in cache:
            cache[key] = Oracle(model_for(models, pore), synth.PORES[pore][0], band)
        exact(cache[key].align(g[p + "signal"], str(g[p + "sequence"]), True), g, p)


def test_g4_dna_long_both_reads(models):
    g = golden("g4_dna_long.npz")
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(int(g["seed"]), int(g["n_reads"]), "dna_r10_400bps", mean, sd, (7000, 8000))
    for i, rd in enumerate(reads):
        assert hashlib.sha256(rd.signal.tobytes()).hexdigest() == str(g[f"r{i}_sha"])
    orc = Oracle(models["syn9"], 4)
    for i, rd in enumerate(reads):  # ~100 k samples each: 2 x ~12 s of oracle time
        exact(orc.align(rd.signal, rd.sequence, True), g, f"r{i}_")


def test_g5_failures_and_messages(models):
    d = json.load(open(os.path.join(GOLDEN, "g5_failures.json")))
    orc = Oracle(models["syn5"], 0)
    for c in d["align"]:
        sig = np.array(c["signal"], dtype=np.float64)
        calc = c["name"] != "calc_false"
        if c["ok"]:
            res = orc.align(sig, c["sequence"], calc)
            assert res["Z"] == c["Z"] and len(res["sequence_positions"]) == c["nseg"]
        else:
            with pytest.raises(RuntimeError) as e:
                orc.align(sig, c["sequence"], calc)
            assert str(e.value) == c["message"]
    for c in d["ctor"]:
        path = {"syn5": models["syn5"], "syn9": models["syn9"]}.get(c["model"], c["model"])
        with pytest.raises(RuntimeError) as e:
            Oracle(path, c["pore"])
        assert str(e.value) == c["message"]


def test_g7_train(models):
    g = golden("g7_train.npz")
    for i in range(int(g["n_cases"])):
        p = f"t{i}_"
        pore = str(g[p + "pore"])
        pid, rna, k = synth.PORES[pore]
        orc = Oracle(model_for(models, pore), pid)
        res = orc.train(g[p + "signal"], str(g[p + "sequence"]))
        assert res["Z"] == float(g[p + "Z"])
        assert np.array_equal(np.array([res["m1"], res["e1"], res["e2"]]), g[p + "trans"])
        mean0, sd0 = orc.table()
        touched = np.nonzero((res["mean"] != mean0) | (res["stdev"] != sd0))[0]
        assert np.array_equal(touched, g[p + "codes"])
        assert np.array_equal(res["mean"][touched], g[p + "mean"])
        assert np.array_equal(res["stdev"][touched], g[p + "stdev"])


def _reference_outputs(models, band=400, pore=3):
    """The compiled reference's outputs: stored in G14 (tests/golden/make_golden_g14.py); where oracle/_ref is built,
    the live reference as well, each compared with the oracle."""
    from oracle import pyoracle
    g = golden("g14_reference_checks.npz")
    return g, (pyoracle.Reference(models["syn9"], pore, band) if pyoracle.reference_available() else None)


def test_oracle_against_compiled_reference_when_present(models):
    g, ref = _reference_outputs(models)
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(991, 4, "dna_r10_260bps", mean, sd, (60, 500))
    assert len(reads) == int(g["short_n"])
    orc = Oracle(models["syn9"], 3)
    mean0, sd0 = orc.table()
    for i, rd in enumerate(reads):
        p = f"short_r{i}_"
        assert hashlib.sha256(rd.signal.tobytes()).hexdigest() == str(g[p + "sha"])
        want_mean, want_sd = mean0.copy(), sd0.copy()
        want_mean[g[p + "codes"]], want_sd[g[p + "codes"]] = g[p + "mean"], g[p + "stdev"]
        stored = {"Z": float(g[p + "Z"]), "probabilities": g[p + "prob"], "signal_positions": g[p + "sigpos"].astype(np.uint64)}
        stored_train = {"m1": float(g[p + "m1"]), "e2": float(g[p + "e2"]), "mean": want_mean, "stdev": want_sd}
        a, ta = orc.align(rd.signal, rd.sequence, True), orc.train(rd.signal, rd.sequence)
        for b, tb in [(stored, stored_train)] + ([(ref.align(rd.signal, rd.sequence, True), ref.train(rd.signal, rd.sequence, orc.num_kmers))] if ref else []):
            assert a["Z"] == b["Z"] and np.array_equal(a["probabilities"], b["probabilities"])
            assert np.array_equal(a["signal_positions"], b["signal_positions"])
            assert ta["m1"] == tb["m1"] and ta["e2"] == tb["e2"]
            assert np.array_equal(ta["mean"], tb["mean"]) and np.array_equal(ta["stdev"], tb["stdev"])


@pytest.mark.parametrize("band,dwell", [(400, 0.5), (100, 0.5), (446, 3.0)])
def test_oracle_against_compiled_reference_dense_long_reads(models, band, dwell):
    """The regime of tests/test_gpu_parity.py::test_dense_reads_moving_window: reads longer than the
    band with 2-3 samples per base (the band window moves in almost every other row)."""
    g, ref = _reference_outputs(models, band, 1)
    j = [(int(b), float(d)) for b, d in zip(g["dense_band"], g["dense_dwell"])].index((band, dwell))
    _, mean, sd = synth.read_model_file(models["syn9"])
    reads = synth.make_reads(99, 3, "rna004", mean, sd, (band + 30, band + 500), dwell=dwell)
    assert len(reads) == int(g[f"dense{j}_n"])
    orc = Oracle(models["syn9"], 1, band)
    for i, rd in enumerate(reads):
        p = f"dense{j}_r{i}_"
        assert hashlib.sha256(rd.signal.tobytes()).hexdigest() == str(g[p + "sha"])
        stored = {"Z": float(g[p + "Z"]), "probabilities": g[p + "prob"], "signal_positions": g[p + "sigpos"].astype(np.uint64),
                  "sequence_positions": g[p + "seqpos"].astype(np.uint64)}
        a = orc.align(rd.signal, rd.sequence, True)
        for b in [stored] + ([ref.align(rd.signal, rd.sequence, True)] if ref else []):
            assert a["Z"] == b["Z"] and np.array_equal(a["probabilities"], b["probabilities"])
            assert np.array_equal(a["signal_positions"], b["signal_positions"])
            assert np.array_equal(a["sequence_positions"], b["sequence_positions"])
