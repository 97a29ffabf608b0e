#!/usr/bin/env python
"""TEST INFRASTRUCTURE (uses the CPU oracle): decision-margin report for a bench workload.

    python tests/decision_margin.py [--workload cfg2] [--reads 1024] [--procs 8] --out profiles/r02/decision_margin_cfg2.json

The integer columns of a segmentation are decided by exact floating-point comparisons in the traceback
(`E[tBb] == M[tBb + eShift] + logScore`, NT_aligner_api.cpp:448, i.e. vM(t-1,n) >= vE(t-1,n)). The GPU
path evaluates the same expressions with its own softplus / emission arithmetic, which differs from
glibc's by rounding errors (~1e-13 accumulated on |vM - vE| at worst). It takes the same decisions as
long as the smallest on-path |vM - vE| is far above that. This script measures that margin with the
oracle over every read of a workload and records the distribution.

Structural ties are reported apart: where two neighbouring lattice columns carry the SAME k-mer (a
homopolymer of k+1 bases -- the polyA pad followed by an A in a quarter of the synthetic RNA reads, any
polyA tail in real data) "enter the column now" and "stay in it" are symmetric, the margin is zero in
exact arithmetic and the reference's own choice rests on rounding noise (0 or ~1e-11, all within the
first ~20 rows here). Those reads are listed so that the GPU parity test compares every one of them.

    python tests/decision_margin.py --family near [--reads 840] [--seed 1] [--replay] --out profiles/imperfect/NAME.json

measures a family of fixture G15 instead (tests/imperfect_families.py; "near" = the six near-duplicate tables, "imperfect" =
every other family, or one family's name), on fresh reads (--seed): per family the floor and percentiles of both margins, the
reads the tie rule (dyn_tie_rows, device="host") flags, and the unflagged reads below 1e-9. With --replay every read also
runs through the CPU replay of strict mode "ties" (tests/tie_parity.py mode 8): reads off the oracle's borders are listed.
"""
from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_O = None


def _init(model, pore_id):
    global _O
    from oracle.pyoracle import Oracle
    _O = Oracle(model, pore_id)


def _work(job):
    sig, seq = job
    r = _O.align(sig, seq, True)
    return _O.last_decision_margin(), len(r["signal_positions"]), _O.last_decision_margin_distinct(), _O.last_decision_margin_at()[:2]


def _fam_init(model, pore_id, band, replay_so):
    global _O, _R
    from oracle.pyoracle import Oracle
    _O = Oracle(model, pore_id, band)
    _R = None
    if replay_so:
        import tie_parity
        _R = tie_parity.Replay(replay_so, model, pore_id, band, mode=8)


def _fam_work(job):
    sig, seq, rows = job
    try:
        r = _O.align(sig, seq, True)
    except RuntimeError:
        return None
    out = [_O.last_decision_margin_distinct(), _O.last_decision_margin_distinct_params(), 0, 0]
    if _R is not None:
        _R.set_strict_rows(rows)
        g = _R.align(sig, seq, True)
        out[2] = int(not (np.array_equal(g["signal_positions"], r["signal_positions"]) and np.array_equal(g["sequence_positions"], r["sequence_positions"])))
        out[3] = int(rows != 0 and g["Z"] != r["Z"])
    return out


def families(a):
    """--family: margins (and the mode-8 replay) over fresh reads of G15's families"""
    import dataclasses
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import imperfect_families as F
    import tie_parity
    from dynamont_amd import Aligner, synth
    names = F.NEAR_FAMILIES if a.family == "near" else F.IMPERFECT_FAMILIES if a.family == "imperfect" else (a.family,)
    tmp = tempfile.mkdtemp(prefix="margin_")
    tables = F.write_tables(tmp)
    so = tie_parity.build_replay(tmp) if a.replay else None
    out = {"what": "fresh reads of fixture G15's families (tests/imperfect_families.py, seed suffix #%d): smallest on-path |vM - vE| between columns "
                   "with different k-mer codes / different (mean, stdev); flagged = dyn_tie_rows != 0; replay = tests/tie_parity.py mode 8 "
                   "(strict mode \"ties\" on the CPU) against the oracle" % a.seed, "families": {}}
    total = {"reads": 0, "flagged": 0, "unflagged_below_1e-9": 0, "unflagged_below_1e-12": 0, "replay_off_the_oracles_borders": 0, "replay_Z_bits_differ_on_flagged_reads": 0}
    for name in names:
        fam = dataclasses.replace(F.FAMILIES[name], name=f"{name}#{a.seed}", n_reads=a.reads or F.FAMILIES[name].n_reads)
        path, mean, sd = tables[fam.table]
        reads = F._GEN[fam.kind](fam, np.asarray(mean), np.asarray(sd))
        al = Aligner(path, fam.pore, band=fam.band, device="host")
        _, _, kms = al.validate([len(r.signal) for r in reads], [r.sequence for r in reads])
        rows = np.array([al.tie_rows(kms[i], len(reads[i].signal)) for i in range(len(reads))], dtype=np.int64)
        al.close()
        with mp.get_context("fork").Pool(a.procs, initializer=_fam_init, initargs=(path, synth.PORES[fam.pore][0], fam.band, so)) as pool:
            res = pool.map(_fam_work, [(r.signal, r.sequence, int(rows[i])) for i, r in enumerate(reads)], chunksize=4)
        ok = np.array([r is not None for r in res])
        mk = np.array([r[0] if r else np.inf for r in res])
        mpar = np.array([r[1] if r else np.inf for r in res])
        unfl = ok & (rows == 0)
        off = [i for i, r in enumerate(res) if r and r[2]]
        rec = {"pore": fam.pore, "table": fam.table, "band": fam.band, "reads": len(reads), "refused": int((~ok).sum()), "flagged": int((rows != 0).sum()),
               "distinct_kmer_decisions": {"min": float(mk[ok].min()), "percentiles": {str(p): float(np.percentile(mk[ok], p)) for p in (1, 10, 50)}},
               "distinct_parameter_decisions": {"min": float(mpar[ok].min()), "percentiles": {str(p): float(np.percentile(mpar[ok], p)) for p in (1, 10, 50)}},
               "unflagged": {"reads": int(unfl.sum()), "min": float(mpar[unfl].min()) if unfl.any() else None,
                             "reads_below_1e-9": int((mpar[unfl] < 1e-9).sum()), "reads_below_1e-12": int((mpar[unfl] < 1e-12).sum())}}
        if a.replay:
            rec["replay_off_the_oracles_borders"] = off
            rec["replay_Z_bits_differ_on_flagged_reads"] = int(sum(r[3] for r in res if r))
            total["replay_off_the_oracles_borders"] += len(off)
            total["replay_Z_bits_differ_on_flagged_reads"] += rec["replay_Z_bits_differ_on_flagged_reads"]
        total["reads"] += len(reads)
        total["flagged"] += rec["flagged"]
        total["unflagged_below_1e-9"] += rec["unflagged"]["reads_below_1e-9"]
        total["unflagged_below_1e-12"] += rec["unflagged"]["reads_below_1e-12"]
        out["families"][name] = rec
        print(name, json.dumps(rec), flush=True)
    if not a.replay:
        del total["replay_off_the_oracles_borders"], total["replay_Z_bits_differ_on_flagged_reads"]
    out["total"] = total
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as w:
        json.dump(out, w, indent=1)
        w.write("\n")
    print(json.dumps(total))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="cfg2")
    ap.add_argument("--family", default="")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--replay", action="store_true")
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--procs", type=int, default=os.cpu_count() or 1)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    if a.family:
        return families(a)
    from dynamont_amd import synth
    cfg = synth.CONFIGS[a.workload]
    pore_id, _, k = synth.PORES[cfg["pore"]]
    tmp = tempfile.mkdtemp(prefix="margin_")
    model = synth.write_model(os.path.join(tmp, f"syn{k}.model"), k, seed=7, stdev=0.25 if k == 5 else 0.15)
    _, mean, sd = synth.read_model_file(model)
    n = a.reads or cfg["n_reads"]
    reads = synth.make_reads(cfg["seed"], n, cfg["pore"], mean, sd, cfg["n_bases"])
    t0 = time.time()
    with mp.get_context("fork").Pool(a.procs, initializer=_init, initargs=(model, pore_id)) as pool:
        res = pool.map(_work, [(r.signal, r.sequence) for r in reads], chunksize=4)
    m = np.array([x[0] for x in res])
    md = np.array([x[2] for x in res])
    segs = int(sum(x[1] for x in res))
    low = [int(i) for i in np.nonzero(m < 1e-6)[0]]
    out = {
        "workload": f"{a.workload}: first {n} reads (seed {cfg['seed']}), {cfg['pore']}, synthetic {k}-mer model",
        "what": "min over on-path traceback decisions of |vM(t-1,n) - vE(t-1,n)| per read (oracle, glibc arithmetic)",
        "reads": int(n), "segments": segs, "decisions": int(sum(len(r.signal) for r in reads)),
        "distinct_kmer_decisions": {"min": float(md.min()), "argmin_read": int(md.argmin()),
                                    "percentiles": {str(p): float(np.percentile(md, p)) for p in (0.1, 1, 10, 50)},
                                    "reads_below_1e-6": int((md < 1e-6).sum())},
        "all_decisions": {"min": float(m.min()), "reads_below_1e-6": len(low), "reads_below_1e-9": int((m < 1e-9).sum()),
                          "percentiles": {str(p): float(np.percentile(m, p)) for p in (0.1, 1, 10, 50)}},
        # reads with a structural tie (same k-mer in neighbouring columns): read index, margin, (row, column), first bases
        "structural_tie_reads": [{"read": i, "margin": float(m[i]), "row_col": list(res[i][3]), "start": reads[i].sequence[:12]} for i in low],
        "wall_s": round(time.time() - t0, 1),
    }
    assert out["distinct_kmer_decisions"]["min"] >= 1e-9, out
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
