"""GPU (-m gpu): dynamont-resquiggle --guide-rescue HW [--guide-rescue-margin M] [--guide-rounds R] end to end, after the pattern
of tests/test_gpu_band_margin_cli.py: ``--band 50 --guide-rescue 16`` writes, for the reads the band margin flags, the bytes of a
``--guide-auto 16`` run and for every other read the bytes of the plain run; the stderr line counts them; --band-report's
``band`` column reads 2 * HW for the rescued reads and the band for the rest, with the margins of the respective run; the three
mutual exclusions end with argparse's error. The flagged set is the library's own on the signals the command aligns
(``Aligner.set_guide_rescue`` on the same handle settings); that set against the CPU is tests/test_gpu_guide_rescue.py's business."""
import os
import uuid

import numpy as np
import pytest

import guide_rescue_cases as rc
import guided_band_cases as gc
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

HW = gc.STALL_HALF_WIDTH
BASE = ["-r", "raw", "-b", "calls.bam", "-o", "out", "--mode", "basic", "-p", "rna004"]


@pytest.mark.parametrize("other, name", [(["--guide-auto", "16"], "--guide-auto"), (["--rescale-iters", "2"], "--rescale-iters"),
                                         (["--border-confidence", "8"], "--border-confidence")])
def test_mutual_exclusions(other, name, capsys):
    with pytest.raises(SystemExit) as e:
        seg.parse(BASE + ["--guide-rescue", "16"] + other)
    assert e.value.code == 2
    assert "--guide-rescue and %s are mutually exclusive" % name in capsys.readouterr().err
    args = seg.parse(BASE + ["--guide-rescue", "16", "--guide-rounds", "4"])
    assert (args.guide_rescue, args.guide_rescue_margin, args.guide_rounds) == (16, 1, 4)
    assert seg.parse(BASE).guide_rescue == 0


def test_resquiggle_guide_rescue(models, tmp_path, capfd):
    _, mean, sd = synth.read_model_file(models["syn5"])
    fam = gc.build_reads(mean, sd)
    reads = fam["a"][:4] + fam["stall"] + fam["a"][4:8]
    lead, seed = 37, 6
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "gr", [synth.SynthRead(r.signal, r.sequence) for r in reads], gc.PORE,
                                             seed=seed, lead=lead, container="pod5", basecalls="bam")

    def run(name, *, batch_reads=7, host=False, report="", **kw):
        out = str(tmp_path / (name + ".csv.zst"))
        capfd.readouterr()
        seg.segment(os.path.dirname(raw), bam, 1, out, models["syn5"], gc.PORE, "basic", minq=0.0, device=0, batch_reads=batch_reads,
                    host_preprocess=host, band=rc.BAND, band_report=report, guide_rounds=8, **kw)
        return zstd_io.decompress(open(out, "rb").read()).decode(), capfd.readouterr().err

    rep = {k: str(tmp_path / (k + ".tsv")) for k in ("rescue", "auto", "plain")}
    text, err = run("rescue", host=True, report=rep["rescue"], guide_rescue=HW)
    auto, _ = run("auto", host=True, report=rep["auto"], guide_auto=HW)
    plain, plain_err = run("plain", host=True, report=rep["plain"])
    # the library's codes on the signals the command aligns (normalised, Hampel-filtered)
    sig, seq = [], []
    for x, s in expected:
        x = x.copy()
        hampel(x)
        sig.append(x)
        seq.append(s)
    al = Aligner(models["syn5"], gc.PORE, band=rc.BAND)
    try:
        al.set_guide_rescue(1, HW, 8)
        res = al.align_batch(sig, seq, True)
    finally:
        al.close()
    codes = res.rescue
    assert set(codes.tolist()) <= {0, 1} and (codes[4:20] == 1).sum() >= 8 and not codes[:4].any() and not codes[20:].any()
    rids = [str(uuid.UUID(int=(seed << 64) | i)) for i in range(len(reads))]
    rows = lambda t: {rid: [ln for ln in t.splitlines()[1:] if ln.startswith(rid + ",")] for rid in rids}  # noqa: E731
    got, want_auto, want_plain = rows(text), rows(auto), rows(plain)
    assert text.splitlines()[0] == plain.splitlines()[0] and len(text.splitlines()) == len(plain.splitlines())
    differ = 0
    for rid, c in zip(rids, codes):
        assert got[rid] and got[rid] == (want_auto[rid] if c == 1 else want_plain[rid]), (rid, int(c))
        differ += c == 1 and want_auto[rid] != want_plain[rid]
    assert differ >= 8                                                     # the rescue changed rows, and only flagged ones
    n1 = int((codes == 1).sum())
    open_ = int(((codes == 1) & (res.guide_converged == 0)).sum())
    assert ("Reads flagged by their band margin (below 1): %d; rescued inside their own guide: %d, of those not converged within 8 "
            "alignments: %d; left as aligned for want of memory: 0, because the rescue failed: 0" % (n1, n1, open_)) in err
    assert "flagged by their band margin" not in plain_err
    # --band-report: 2 * HW and the guided margins for the rescued reads, the band and the diagonal margins for the rest
    lines = {k: {ln.split("\t")[0]: ln.split("\t") for ln in open(v).read().split("\n")[1:-1]} for k, v in rep.items()}
    assert sorted(lines["rescue"]) == sorted(rids)
    for rid, c in zip(rids, codes):
        f = lines["rescue"][rid]
        assert f[3] == (str(2 * HW) if c == 1 else str(rc.BAND)), rid
        assert f == (lines["auto"][rid] if c == 1 else lines["plain"][rid]), rid
    # preprocessing on the device (the BAM-columns front end), and the whole run as one ticket: the same bytes again
    report2 = str(tmp_path / "rescue2.tsv")
    text2, err2 = run("device", report=report2, guide_rescue=HW)
    assert text2 == text and open(report2).read() == open(rep["rescue"]).read()
    assert "rescued inside their own guide: %d," % n1 in err2
    assert run("one", batch_reads=64, guide_rescue=HW)[0] == text
    # a margin of 0 flags nothing: the plain run's bytes
    text0, err0 = run("zero", guide_rescue=HW, guide_rescue_margin=0)
    assert text0 == plain and "Reads flagged by their band margin (below 0): 0; rescued inside their own guide: 0," in err0
