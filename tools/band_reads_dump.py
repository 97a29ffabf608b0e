#!/usr/bin/env python
"""GPU box: every output array of the banded-lattice kernel (band_reads.hip) on a fixed case list, for a bit-for-bit comparison
of two builds of the library. Only the public Python API is used, so the same file runs on any commit that has the guided band.

    python tools/band_reads_dump.py OUT.npz          run the cases, write every array
    python tools/band_reads_dump.py --compare A B    per array: array_equal on integer / uint64 views; exit status 1 on a difference

Cases
  wide    rna004 (syn9), bands 600 and 1 000, four reads each (two long ones, one of them behind a polyA run, and two whose half
          band is N / 2): align, the Z-only call, train; at band 600 also border confidence (W = 8) and segment scores (W = 8)
  guided  dna_r9 (syn5), a diagonal guide at half widths 12, 100 and 135 (one per kernel shape): align, Z only, train; the stalled
          reads of tests/guided_band_cases.py at half width 16 with set_guide_refine(4): results, guide() and guide_rounds()"""
import os, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ALIGN = ("Z", "status", "seg_offsets", "n_segments", "sequence_positions", "signal_positions", "probabilities", "states")
TRAIN = ("Z", "status", "transitions", "em_offsets", "em_count", "em_code", "em_mean", "em_stdev", "em_weight", "em_sum", "em_sumsq",
         "trans_counts")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.view(np.uint32) if a.dtype == np.float32 else a


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    bad = 0
    for k in sorted(set(A.files) | set(B.files)):
        if k not in A.files or k not in B.files:
            print("%-48s only in %s" % (k, pa if k in A.files else pb))
            bad += 1
            continue
        eq = A[k].shape == B[k].shape and A[k].dtype == B[k].dtype and np.array_equal(bits(A[k]), bits(B[k]))
        print("%-48s %-8s %-12s %s" % (k, A[k].dtype, A[k].shape, "equal" if eq else "DIFFERENT"))
        bad += not eq
    print("%d arrays, %d different" % (len(set(A.files) | set(B.files)), bad))
    return 1 if bad else 0


def wide_reads(synth, mean, sd, band):
    """two reads longer than the band (one behind a polyA run) and two whose half band is N / 2 (N odd and even)"""
    n = band + 28
    reads = synth.make_reads(9100 + band, 1, "rna004", mean, sd, (n, n + 80))
    reads += synth.make_reads(9200 + band, 1, "rna004", mean, sd, (n, n + 80), polya=(20, 60))
    half = band // 2
    reads += synth.make_reads(9300 + band, 1, "rna004", mean, sd, 2 * (half - 50) + 8)        # N = 2 (half - 50) + 1
    reads += synth.make_reads(9400 + band, 1, "rna004", mean, sd, 2 * (half - 20) + 7)        # N = 2 (half - 20)
    return reads


def dump(out_path):
    import guided_band_cases as gc
    from dynamont_amd import Aligner, synth
    out = {}

    def put(case, res, names):
        for nm in names:
            v = getattr(res, nm)
            if v is not None:
                out["%s/%s" % (case, nm)] = np.asarray(v).copy()

    d = tempfile.mkdtemp()
    m9 = synth.write_model(os.path.join(d, "syn9.model"), 9, seed=7, stdev=0.15)
    _, mean9, sd9 = synth.read_model_file(m9)
    for band in (600, 1000):
        reads = wide_reads(synth, mean9, sd9, band)
        sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
        al = Aligner(m9, "rna004", band=band, device=0)
        put("wide%d/align" % band, al.align_batch(sig, seq, True), ALIGN)
        put("wide%d/zonly" % band, al.align_batch(sig, seq, False), ALIGN)
        put("wide%d/train" % band, al.train_batch(sig, seq), TRAIN)
        if band == 600:
            al.set_border_confidence(8)
            al.set_segment_scores(8)
            put("wide600/riders", al.align_batch(sig, seq, True),
                ALIGN + ("border_probability", "border_window_probability", "median_delta", "mad_delta", "homogeneity"))
        al.close()

    m5 = synth.write_model(os.path.join(d, "syn5.model"), 5, seed=7, stdev=0.25)
    _, mean5, sd5 = synth.read_model_file(m5)
    fam = gc.build_reads(mean5, sd5)
    al = Aligner(m5, gc.PORE, band=50, device=0)
    for hw, reads in ((12, fam["a"][:6]), (100, [r for r in fam["a"] if r.n_kmers + 1 >= 201][:6]), (135, fam["a2"])):
        sig, seq = [r.signal for r in reads], [r.sequence for r in reads]
        guides = [gc.diagonal(r) for r in reads]
        put("guided%d/align" % hw, al.align_batch_guided(sig, seq, guides, hw), ALIGN)
        put("guided%d/zonly" % hw, al.align_batch_guided(sig, seq, guides, hw, calc_probabilities=False), ALIGN)
        put("guided%d/train" % hw, al.train_batch_guided(sig, seq, guides, hw), TRAIN)
    stall = fam["stall"]
    sig, seq = [r.signal for r in stall], [r.sequence for r in stall]
    guides = [gc.diagonal(r) if i % 2 == 0 else gc.true_guide(r) for i, r in enumerate(stall)]
    res = al.align_batch_guided(sig, seq, guides, 16, refine=4)
    put("refine16/align", res, ALIGN + ("guide_rounds", "guide_converged"))
    out["refine16/guide"] = np.concatenate(res.guides)
    al.close()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    np.savez(out_path, **out)
    print("%d arrays -> %s" % (len(out), out_path))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
