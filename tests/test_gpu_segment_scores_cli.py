"""GPU (-m gpu): dynamont-resquiggle --segment-scores 8, with and without --event-stats. The columns before the new ones and
`.errors` are those of a run without the flag; the header gains the three names; every row's three fields are Python's
f"{v:.6f}" of the restatement (tests/segment_scores_cases.py) over the normalised, Hampel-filtered signal; the Python
formatting path (--parallel-zstd-frames) writes the same bytes; the output without the flag is that of a run that never heard
of it."""
import os

import pytest

import segment_scores_cases as ssc
from conftest import model_for
from dynamont_amd import synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

PORE = "rna004"
W = 8
NAMES = ",median_delta,mad_delta,homogeneity"


def _run(model, raw, bam, out, *extra):
    seg.main(["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", PORE, "--model_path", model,
              "--batch-reads", "4", "-o", str(out)] + list(extra))
    data = open(str(out) + ".zst", "rb").read()
    errors = os.path.splitext(str(out))[0] + ".errors"
    return zstd_io.decompress(data).decode(), open(errors).read() if os.path.exists(errors) else ""


def test_score_columns_with_and_without_levels(models, tmp_path):
    model = model_for(models, PORE)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(7401, 12, PORE, mean, sd, (60, 220))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "sc", reads, PORE, seed=3, basecalls="tsv")
    lines = open(bam).read().splitlines()   # one read that fails in the aligner: its .errors line must not change
    f = lines[4].split("\t"); f[1] = f[1][:30] + "N" + f[1][31:]; lines[4] = "\t".join(f)
    open(bam, "w").write("\n".join(lines) + "\n")

    plain, plain_err = _run(model, raw, bam, tmp_path / "plain.csv")
    assert seg.parse(["-r", "x", "-b", "y", "--mode", "basic", "-p", PORE, "--model_path", model, "-o", "z"]).segment_scores == 0
    levels, _ = _run(model, raw, bam, tmp_path / "levels.csv", "--event-stats")
    for base, base_text, extra in (("plain", plain, []), ("levels", levels, ["--event-stats"])):
        text, err = _run(model, raw, bam, tmp_path / f"{base}_sc.csv", "--segment-scores", str(W), *extra)
        assert err == plain_err and plain_err.count("\n") >= 1
        b_lines, s_lines = base_text.splitlines(), text.splitlines()
        assert s_lines[0] == b_lines[0] + NAMES and len(b_lines) == len(s_lines) > 300
        rows = {}
        for b, s in zip(b_lines[1:], s_lines[1:]):
            f = s.split(",")
            assert ",".join(f[:-3]) == b                    # everything before the new columns: the run without the flag
            rows.setdefault(f[0], []).append(f)
        for rid, fs in rows.items():
            x = expected[int(rid.rsplit("-", 1)[1])][0].copy()
            hampel(x)   # the CLI aligns the Hampel-filtered signal
            s0 = int(fs[0][2])
            assert int(fs[-1][3]) - s0 == len(x)
            want = ssc.scores(x, [int(f[2]) - s0 for f in fs], W)
            assert fs[0][-3:-1] == ["nan", "nan"]
            for j, f in enumerate(fs):
                assert f[-3:] == [f"{want[0, j]:.6f}", f"{want[1, j]:.6f}", f"{want[2, j]:.6f}"], (base, rid, j)
        if extra:   # the Python formatting path: the same bytes
            other, other_err = _run(model, raw, bam, tmp_path / "frames.csv", "--segment-scores", str(W), *extra, "--parallel-zstd-frames")
            assert other == text and other_err == err
    # without the flag: the same bytes again, and the same compressed file
    again, again_err = _run(model, raw, bam, tmp_path / "again.csv", "--segment-scores", "0")
    assert again == plain and again_err == plain_err
    assert open(tmp_path / "again.csv.zst", "rb").read() == open(tmp_path / "plain.csv.zst", "rb").read()
