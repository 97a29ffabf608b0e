"""TEST INFRASTRUCTURE (uses the CPU oracle; run by hand on a GPU box, not collected by pytest):

    python tests/fuzz_parity.py [seed = 20261004] [reads per pore and band = 150] > gpurun_out/fuzz.txt

3 000 random short reads (k .. 400 bases, dwell 0.5 .. 10) over the five pore types and four random band widths each
against the oracle: integer columns identical, posteriors within 1e-6, Z within 1e-9 relative, failures with the
reference's message; round 3 also train() (Z, transitions, per-k-mer weights at 1e-7 relative, weights summing to the
sample count) and align(calc=false) on the same reads. Round 2: 0 mismatches (profiles/r02/fuzz_parity_3000_reads.txt);
round 3, final build: profiles/r03/fuzz_parity_3000_reads.txt.

    python tests/fuzz_parity.py --imperfect [seed = 20261017] [reads per pore and table = 1000] > fuzz_imperfect.txt

draws every read from the generators of fixture G15 instead (tests/imperfect_families.py: random_read -- a random family per
read: basecalling errors under Poisson or heavy-tailed dwell, the seven stress variants, far-out samples), on the four pores'
ordinary tables and on the six near-duplicate tables, handle as created: status and message, integer columns, Z (bit for bit
on reads the tie rule flags), posteriors and the Z-only call against the oracle."""
import os, sys, tempfile, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamont_amd import Aligner, synth
from oracle.pyoracle import Oracle


def _imperfect(argv):
    import multiprocessing as mp
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import imperfect_families as F
    seed = int(argv[0]) if argv else 20261017
    per = int(argv[1]) if len(argv) > 1 else 1000
    rng = np.random.default_rng(seed)
    tables = F.write_tables(tempfile.mkdtemp())
    groups = [(p, F.table_for(p)) for p in F.PORES] + [(F.FAMILIES[n].pore, F.FAMILIES[n].table) for n in F.NEAR_FAMILIES]
    tot = bad = bad_z = bad_p = bad_zonly = refused = flagged = 0
    for pore, table in groups:
        path, mean, sd = tables[table]
        drawn = [F.random_read(rng, pore, mean, sd, near=table.startswith("near")) for _ in range(per)]
        reads = [d[0] for d in drawn]
        sigs, seqs = [r.signal for r in reads], [r.sequence for r in reads]
        al = Aligner(path, pore, device=0)
        res = al.align_batch(sigs, seqs, True)
        zs = al.align_batch(sigs, seqs, False)
        _, _, kms = al.validate([len(x) for x in sigs], seqs)
        rows = [al.tie_rows(kms[i], len(sigs[i])) for i in range(per)]
        al.close()
        with mp.get_context("fork").Pool(min(16, os.cpu_count() or 1), initializer=_orc_start, initargs=(path, synth.PORES[pore][0])) as pool:
            want = pool.map(_orc_full, list(zip(sigs, seqs)), chunksize=4)
        for i, w in enumerate(want):
            fam, noisy = drawn[i][1], drawn[i][2]
            if isinstance(w, str):
                refused += 1
                if res.error(i) != w or zs.error(i) != w:
                    bad += 1
                    print("MESSAGE MISMATCH", pore, table, fam, i, res.error(i), zs.error(i), w, flush=True)
                continue
            tot += 1
            flagged += rows[i] != 0
            if res.status[i] != 0:
                bad += 1
                print("REFUSED BY THE DEVICE ONLY", pore, table, fam, i, res.error(i), flush=True)
                continue
            got = res.read(i)
            if not (np.array_equal(got["sequence_positions"], w[1]) and np.array_equal(got["signal_positions"], w[0])):
                bad += 1
                print("MISMATCH", pore, table, fam, i, len(seqs[i]), len(sigs[i]), "tie_rows", rows[i], flush=True)
                continue
            if not (got["Z"] == w[2] if rows[i] else abs(got["Z"] - w[2]) <= 1e-9 * max(1.0, abs(w[2]))):
                bad_z += 1
                print("Z MISMATCH", pore, table, fam, i, got["Z"], w[2], "tie_rows", rows[i], flush=True)
            if np.abs(got["probabilities"] - w[3]).max() > (max(1e-6, 1024 * 2.2e-16 * abs(w[2])) if noisy else 1e-6):
                bad_p += 1
                print("POSTERIOR MISMATCH", pore, table, fam, i, float(np.abs(got["probabilities"] - w[3]).max()), w[2], flush=True)
            if not (zs.status[i] == 0 and abs(zs.Z[i] - w[2]) <= 1e-9 * max(1.0, abs(w[2]))):
                bad_zonly += 1
                print("Z-ONLY MISMATCH", pore, table, fam, i, flush=True)
        print(pore, table, "done", tot, bad, bad_z, bad_p, bad_zonly, refused, flush=True)
    print("TOTAL imperfect reads compared", tot, "of them flagged by the tie rule", flagged, "integer or message mismatches", bad, "Z mismatching", bad_z,
          "posteriors mismatching", bad_p, "Z-only mismatching", bad_zonly, "refusals reproduced", refused)


_ORC = {}


def _orc_start(model, pore_id):
    _ORC["o"] = Oracle(model, pore_id, 400)


def _orc_full(job):
    try:
        r = _ORC["o"].align(job[0], job[1], True)
    except RuntimeError as e:
        return str(e)
    return r["signal_positions"], r["sequence_positions"], r["Z"], r["probabilities"]


if "--imperfect" in sys.argv:
    _imperfect([a for a in sys.argv[1:] if a != "--imperfect"])
    sys.exit(0)
d = tempfile.mkdtemp()
SEED = int(sys.argv[1]) if len(sys.argv) > 1 else 20261004
PER = int(sys.argv[2]) if len(sys.argv) > 2 else 150
rng = np.random.default_rng(SEED)
tot = bad = err = bad_train = bad_z = 0
for pore in ("rna002", "rna004", "dna_r9", "dna_r10_260bps", "dna_r10_400bps"):
    k = synth.PORES[pore][2]
    path = synth.write_model(os.path.join(d, f"{pore}.model"), k)
    _, mean, sd = synth.read_model_file(path)
    for band in (int(x) for x in rng.choice([6, 16, 50, 100, 200, 300, 400, 446], 4, replace=False)):
        reads = []
        for i in range(PER):
            nb = int(rng.integers(k, 400))
            reads += synth.make_reads(int(rng.integers(1 << 30)), 1, pore, mean, sd, nb, dwell=float(rng.choice([0.5, 2.0, 3.5, 7.0, 10.0])))
        al = Aligner(path, pore, band=band, device=0)
        orc = Oracle(path, synth.PORES[pore][0], band)
        res = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
        zs = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], False)
        tr = al.train_batch([r.signal for r in reads], [r.sequence for r in reads])
        for i, r in enumerate(reads):
            try:
                want = orc.align(r.signal, r.sequence, True)
            except RuntimeError as e:
                err += 1
                assert res.error(i) == str(e), (pore, band, i, res.error(i), str(e))
                continue
            tot += 1
            got = res.read(i)
            ok = res.status[i] == 0 and np.array_equal(got["sequence_positions"], want["sequence_positions"]) and np.array_equal(got["signal_positions"], want["signal_positions"])
            if ok:
                ok = np.abs(got["probabilities"] - want["probabilities"]).max() <= 1e-6 and abs(got["Z"] - want["Z"]) <= 1e-9 * max(1.0, abs(want["Z"]))
            if not ok:
                bad += 1
                print("MISMATCH", pore, band, i, len(r.sequence), len(r.signal), flush=True)
            if not (zs.status[i] == 0 and abs(zs.Z[i] - want["Z"]) <= 1e-9 * max(1.0, abs(want["Z"]))):
                bad_z += 1
                print("Z-ONLY MISMATCH", pore, band, i, flush=True)
            wt = orc.train(r.signal, r.sequence, dense=False)
            code, m, _ = tr.sparse(i)
            a = int(tr.em_offsets[i])
            touched = np.nonzero(wt["weight"] > 0)[0]
            okt = tr.status[i] == 0 and abs(tr.Z[i] - wt["Z"]) <= 1e-9 * max(1.0, abs(wt["Z"])) and np.array_equal(code, touched)
            if okt:
                gw = tr.em_weight[a:a + len(code)]
                okt = np.allclose(gw, wt["weight"][touched], rtol=1e-7, atol=1e-12) and abs(gw.sum() - len(r.signal)) <= 1e-9 * len(r.signal)
                okt = okt and abs(tr.transitions[3 * i] - wt["m1"]) <= 1e-8 and abs(tr.transitions[3 * i + 2] - wt["e2"]) <= 1e-8
            if not okt:
                bad_train += 1
                print("TRAIN MISMATCH", pore, band, i, len(r.sequence), len(r.signal), flush=True)
        print(pore, band, "done", tot, bad, bad_z, bad_train, err, flush=True)
        al.close()
print("TOTAL reads compared", tot, "align mismatching", bad, "Z-only mismatching", bad_z, "train mismatching", bad_train, "expected errors reproduced", err)
