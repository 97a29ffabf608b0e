#!/usr/bin/env python
"""TEST INFRASTRUCTURE (CPU only, run by hand): what widening the tie rule to near-duplicate parameters costs.

    python tests/tie_rule_cost.py --out profiles/imperfect/tie_rule_flagged_counts.json

dyn_tie_rows (device="host") flags a read when two neighbouring columns lie within 1e-9 of each other in mean and stdev; before
fixture G15 it asked for bit-equal parameters. A flagged read costs ~1.2x a plain one, so the bench workloads must not flag
more reads than they did: for every read of cfg2, cfg2_polya and cfg3 and of the G10, G12 and G13 families this counts the
reads the library flags and the reads with a bit-equal neighbouring pair (the old rule, restated in NumPy)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import imperfect_families as F  # noqa: E402
import tie_parity  # noqa: E402
from dynamont_amd import Aligner, synth  # noqa: E402


def count(model, pore, reads):
    al = Aligner(model, pore, device="host")
    mean_c, sd_c = al.model_table()
    new = old = 0
    for a in range(0, len(reads), 512):
        part = reads[a:a + 512]
        _, _, kms = al.validate([len(r.signal) for r in part], [r.sequence for r in part])
        for r, k in zip(part, kms):
            new += al.tie_rows(k, len(r.signal)) != 0
            old += bool(len(k) > 1 and (F.pair_gaps(k, mean_c, sd_c) == 0).any())
    al.close()
    return {"reads": len(reads), "flagged": int(new), "flagged_by_bit_equal_parameters": int(old)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="tie_cost_")
    out = {}
    syn = {5: synth.write_model(os.path.join(tmp, "syn5.model"), 5, seed=7, stdev=0.25), 9: synth.write_model(os.path.join(tmp, "syn9.model"), 9, seed=7, stdev=0.15)}
    for wl in ("cfg2", "cfg2_polya", "cfg3"):
        cfg = synth.CONFIGS[wl]
        model = syn[synth.PORES[cfg["pore"]][2]]
        _, mean, sd = synth.read_model_file(model)
        out[wl] = count(model, cfg["pore"], synth.make_reads(cfg["seed"], cfg["n_reads"], cfg["pore"], mean, sd, cfg["n_bases"], polya=cfg.get("polya")))
        print(wl, out[wl], flush=True)
    for tag, paths, fams in (("g10", tie_parity.g10_model_paths(tmp), tie_parity.G10_FAMILIES), ("g12", tie_parity.g12_model_paths(tmp), tie_parity.G12_FAMILIES)):
        for fam, (pore, mkey, gen) in fams.items():
            _, mean, sd = synth.read_model_file(paths[mkey])
            out[f"{tag}_{fam}"] = count(paths[mkey], pore, gen(mean, sd))
            print(tag, fam, out[f"{tag}_{fam}"], flush=True)
    g = np.load(os.path.join(ROOT, "tests", "golden", "g13_margin_families.npz"), allow_pickle=False)
    from test_gpu_parity import _g13_clustered9
    for fam, spec in json.loads(str(g["families"])).items():
        pore = spec["pore"]
        if spec["table"] == "syn9":
            model = syn[9]
        else:
            mean, sd = _g13_clustered9(g["rna004_5_mean"], g["rna004_5_sd"]) if spec["table"] == "clustered9" else (g[spec["table"] + "_mean"], g[spec["table"] + "_sd"])
            model = synth.write_model_values(os.path.join(tmp, f"{fam}.model"), synth.PORES[pore][2], mean, sd)
        _, mean, sd = synth.read_model_file(model)
        out[f"g13_{fam}"] = count(model, pore, synth.make_reads(spec["seed"], spec["reads"], pore, np.asarray(mean), np.asarray(sd), tuple(spec["bases"])))
        print("g13", fam, out[f"g13_{fam}"], flush=True)
    changed = {k: v for k, v in out.items() if v["flagged"] != v["flagged_by_bit_equal_parameters"]}
    rec = {"what": "reads flagged by dyn_tie_rows (neighbouring columns within 1e-9 in mean and stdev) against reads with a bit-equal neighbouring pair "
                   "(the rule before fixture G15)", "workloads": out, "workloads_whose_flagged_count_changed": sorted(changed)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as w:
        json.dump(rec, w, indent=1)
        w.write("\n")
    print("changed:", sorted(changed))


if __name__ == "__main__":
    main()
