#!/usr/bin/env python
"""Generate golden fixture G15 -- align() on IMPERFECT READS and on NEAR-DUPLICATE TABLES -- and
profiles/imperfect/decision_margins.json. Needs the compiled reference (`make -C oracle ref`) and the built library (the tie
rule is asked of a device="host" handle).

    python tests/golden/make_golden_g15.py [workers]

Every other align() fixture draws the signal from the read's own bases with Poisson dwell. The families here
(tests/imperfect_families.py) are what real data adds: basecalls with 2/1, 5/3 and 10/6 % substitutions / indels under Poisson
and under heavy-tailed dwell with stalls; the seven stress variants of the train() tests (spiky, far-out, permuted, reversed,
flat, squeezed, mis-called); samples at 1e4 and 2e5; cfg2-shaped reads of 2 000 bases; the squeezed and the 10/6 % family again
at band 50, where the path leaves the band; band 600 on reads of 470+ bases (the generic wide-band kernel); and six tables whose
neighbouring k-mers lie 1e-6 .. 1e-16 apart in mean or stdev (synth.near_duplicate_table), where the traceback's on-path margin
is NOT far above the arithmetic's noise and the tie rule (bit-equal parameters only) does not flag the read.

Per read: the COMPILED REFERENCE's borders, Z, status and message (a refused read is recorded data); the oracle's two margins
(smallest on-path |vM - vE| between distinct k-mer codes / between columns with different parameters); dyn_tie_rows; len(signal)
and a CRC of its bytes. Reference and oracle run side by side and must agree bit for bit while generating. Inputs are
regenerated from seeds, never stored. The file is written with fixed zip timestamps: regenerating gives the same bytes."""
from __future__ import annotations

import io
import json
import multiprocessing as mp
import os
import sys
import tempfile
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imperfect_families as F  # noqa: E402
from dynamont_amd import Aligner, synth  # noqa: E402
from oracle.pyoracle import Oracle, Reference  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
MAX_REFUSED = 0.10

_W = {}


def _init(model, pore, band):
    enum = synth.PORES[pore][0]
    _W["ref"] = Reference(model, enum, band)
    _W["orc"] = Oracle(model, enum, band)


def _one(job):
    sig, seq = job
    try:
        want = _W["ref"].align(sig, seq, True)
    except RuntimeError as e:
        try:
            _W["orc"].align(sig, seq, True)
        except RuntimeError as e2:
            assert str(e2) == str(e), (str(e), str(e2))
            return None, None, float("nan"), str(e), float("inf"), float("inf"), True
        raise AssertionError("the reference refuses a read the oracle aligns: " + str(e))
    got = _W["orc"].align(sig, seq, True)
    assert np.array_equal(want["signal_positions"], got["signal_positions"]) and np.array_equal(want["sequence_positions"], got["sequence_positions"])
    assert want["Z"] == got["Z"]
    return (np.asarray(want["signal_positions"], dtype=np.int32), np.asarray(want["sequence_positions"], dtype=np.int32), float(want["Z"]), "",
            float(_W["orc"].last_decision_margin_distinct()), float(_W["orc"].last_decision_margin_distinct_params()),
            all(s == "M" for s in want["states"]))


def save_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def _stats(m):
    fin = m[np.isfinite(m)]
    if not len(fin):
        return {"min": None, "percentiles": {}, "reads_below_1e-6": 0, "reads_below_1e-9": 0, "reads_below_1e-12": 0}
    return {"min": float(fin.min()), "argmin_read": int(np.argmin(np.where(np.isfinite(m), m, np.inf))),
            "percentiles": {str(p): float(np.percentile(fin, p)) for p in (1, 10, 50)},
            "reads_below_1e-6": int((fin < 1e-6).sum()), "reads_below_1e-9": int((fin < 1e-9).sum()), "reads_below_1e-12": int((fin < 1e-12).sum())}


def main():
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else min(16, os.cpu_count() or 1)
    tmp = tempfile.mkdtemp(prefix="g15_")
    tables = F.write_tables(tmp)
    fixture = {}
    sweep_gap, sweep_margin = [], []
    report = {"what": "per family of tests/golden/g15_imperfect_reads.npz: min over on-path traceback decisions of |vM(t-1,n) - vE(t-1,n)| "
                      "(oracle = compiled reference bit for bit) between columns with different k-mer CODES (distinct_kmer_decisions) and "
                      "between columns whose (mean, stdev) differ (distinct_parameter_decisions: the decisions of reads the tie rule leaves "
                      "unflagged); flagged = reads with dyn_tie_rows != 0",
              "families": {}}
    for name, fam in F.FAMILIES.items():
        path = tables[fam.table][0]
        reads = F.reads_of(name, tables)
        with mp.get_context("fork").Pool(workers, initializer=_init, initargs=(path, fam.pore, fam.band)) as pool:
            res = pool.map(_one, [(r.signal, r.sequence) for r in reads], chunksize=1)
        al = Aligner(path, fam.pore, band=fam.band, device="host")
        _, _, kms = al.validate([len(r.signal) for r in reads], [r.sequence for r in reads])
        rows = np.array([al.tie_rows(kms[i], len(reads[i].signal)) for i in range(len(reads))], dtype=np.uint32)
        mean_c, sd_c = al.model_table()
        al.close()
        # the closest neighbouring pair of columns of every read (0: equal parameters, the tie rule before G15)
        gap = np.array([F.pair_gaps(k, mean_c, sd_c).min() if len(k) > 1 else np.inf for k in kms])
        assert np.array_equal(rows != 0, gap <= F.TIE_TAU), name     # the library's rule is the one the sweep below chose
        if fam.kind in ("near", "found"):
            sweep_gap.append(gap[~np.array([r[0] is None for r in res])])
            sweep_margin.append(np.array([r[5] for r in res if r[0] is not None]))
        refused = np.array([r[0] is None for r in res])
        assert refused.mean() <= MAX_REFUSED, (name, int(refused.sum()), "change the family's parameters, not the cap")
        offs = np.zeros(len(reads) + 1, dtype=np.int64)
        np.cumsum([0 if r[0] is None else len(r[0]) for r in res], out=offs[1:])
        empty = np.zeros(0, dtype=np.int32)
        fixture[f"{name}_sigpos"] = np.concatenate([empty if r[0] is None else r[0] for r in res])
        fixture[f"{name}_seqpos"] = np.concatenate([empty if r[1] is None else r[1] for r in res])
        fixture[f"{name}_seg_off"] = offs
        fixture[f"{name}_Z"] = np.array([r[2] for r in res])
        fixture[f"{name}_status"] = refused.astype(np.int8)
        fixture[f"{name}_message"] = np.array([r[3] for r in res])
        mk = np.array([r[4] for r in res])
        mpar = np.array([r[5] for r in res])
        fixture[f"{name}_margin_kmer"] = mk
        fixture[f"{name}_margin_params"] = mpar
        fixture[f"{name}_all_M"] = np.array([bool(r[6]) for r in res])
        fixture[f"{name}_rows"] = rows
        fixture[f"{name}_bit_equal_tie"] = gap == 0
        fixture[f"{name}_S"] = np.array([len(r.signal) for r in reads], dtype=np.int32)
        fixture[f"{name}_crc"] = np.array([F.signal_crc(r) for r in reads], dtype=np.uint32)
        unflagged = (rows == 0) & ~refused
        report["families"][name] = {
            "pore": fam.pore, "table": fam.table, "band": fam.band, "kind": fam.kind, "reads": len(reads), "refused": int(refused.sum()),
            "samples": int(sum(len(r.signal) for r in reads)), "segments": int(offs[-1]), "flagged": int((rows != 0).sum()),
            "flagged_by_bit_equal_parameters": int((gap == 0).sum()),
            "distinct_parameter_decisions": _stats(mpar), "distinct_kmer_decisions": _stats(mk),
            "unflagged": {"reads": int(unflagged.sum()), **_stats(mpar[unflagged])}}
        print(name, json.dumps(report["families"][name]), flush=True)
    # The tie rule's threshold, from the reference alone: flag a read when two neighbouring columns lie within tau of each other
    # in mean and stdev; over the near-duplicate families, the smallest decade at which every read left unflagged keeps an
    # on-path margin >= 1e-9
    gap, margin = np.concatenate(sweep_gap), np.concatenate(sweep_margin)
    sweep = []
    for e in range(16, 5, -1):
        un = gap > 10.0 ** -e
        sweep.append({"tau": f"1e-{e}", "unflagged_reads": int(un.sum()), "of": int(len(gap)),
                      "unflagged_margin_floor": float(margin[un].min()) if un.any() else None, "unflagged_below_1e-9": int((margin[un] < 1e-9).sum())})
    chosen = next(s["tau"] for s in sweep if s["unflagged_below_1e-9"] == 0)
    assert float(chosen) == F.TIE_TAU, chosen
    report["tie_rule_sweep"] = {"what": "near-duplicate families of G15 together: reads with no neighbouring pair of columns within tau (max of |d mean|, "
                                        "|d stdev|) and the floor of their parameter-distinct margin; chosen = the smallest decade with no such read below 1e-9 "
                                        "= dyn_tie_rows' TIE_TAU", "sweep": sweep, "chosen_tau": chosen}
    fixture["families"] = np.array(json.dumps(list(F.FAMILIES)))
    out = os.path.join(OUT, "g15_imperfect_reads.npz")
    save_npz(out, fixture)
    os.makedirs(os.path.join(ROOT, "profiles", "imperfect"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "imperfect", "decision_margins.json"), "w") as w:
        json.dump(report, w, indent=1)
        w.write("\n")
    print("written", os.path.getsize(out), "bytes")
    assert os.path.getsize(out) <= 1000000


if __name__ == "__main__":
    main()
