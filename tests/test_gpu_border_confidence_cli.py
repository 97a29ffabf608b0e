"""GPU (-m gpu): dynamont-resquiggle --border-confidence 8 on two small datasets. The header gains the two names, every row's
two fields are Python's f"{x:.6f}" of what the API returns for the same read (Aligner.set_border_confidence over the
normalised, Hampel-filtered signal), everything before them and `.errors` are those of a run without the flag, and without
the flag the output is that of a run that never heard of it."""
import os

import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

W = 8
NAMES = ",border_probability,border_window_probability"


def _run(model, pore, raw, bam, out, *extra):
    seg.main(["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", pore, "--model_path", model,
              "--batch-reads", "4", "-o", str(out)] + list(extra))
    data = open(str(out) + ".zst", "rb").read()
    errors = os.path.splitext(str(out))[0] + ".errors"
    return zstd_io.decompress(data).decode(), open(errors).read() if os.path.exists(errors) else ""


@pytest.mark.parametrize("pore,seed", [("rna004", 7501), ("dna_r10_400bps", 7502)])
def test_border_columns_equal_the_api(models, tmp_path, pore, seed):
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(seed, 10, pore, mean, sd, (60, 220))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "bc", reads, pore, seed=3, basecalls="tsv")

    plain, plain_err = _run(model, pore, raw, bam, tmp_path / "plain.csv")
    text, err = _run(model, pore, raw, bam, tmp_path / "bc.csv", "--border-confidence", str(W))
    assert err == plain_err
    b_lines, s_lines = plain.splitlines(), text.splitlines()
    assert s_lines[0] == b_lines[0] + NAMES and len(b_lines) == len(s_lines) > 300
    rows = {}
    for b, s in zip(b_lines[1:], s_lines[1:]):
        f = s.split(",")
        assert ",".join(f[:-2]) == b                    # everything before the new columns: the run without the flag
        rows.setdefault(f[0], []).append(f)
    assert len(rows) == len(reads)
    al = Aligner(model, pore, device=0)
    al.set_border_confidence(W)
    order = sorted(rows, key=lambda rid: int(rid.rsplit("-", 1)[1]))
    sigs = []
    for rid in order:
        x = expected[int(rid.rsplit("-", 1)[1])][0].copy()
        hampel(x)   # the CLI aligns the Hampel-filtered signal
        sigs.append(x)
    res = al.align_batch(sigs, [expected[int(rid.rsplit("-", 1)[1])][1] for rid in order], True)
    assert (res.status == 0).all()
    below_one = 0
    for i, rid in enumerate(order):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        fs = rows[rid]
        assert len(fs) == m
        for j, f in enumerate(fs):
            assert f[-2:] == [f"{res.border_probability[a + j]:.6f}", f"{res.border_window_probability[a + j]:.6f}"], (rid, j)
            below_one += f[-1] != "1.000000"
    assert below_one >= 10                               # the columns carry information, not a constant
    al.close()
    # with both other opt-ins as well: the two columns come last, after theirs
    both, _ = _run(model, pore, raw, bam, tmp_path / "all.csv", "--event-stats", "--segment-scores", "8", "--border-confidence", str(W))
    a_lines = both.splitlines()
    assert a_lines[0] == b_lines[0] + ",level_mean,level_stdv,level_median,median_delta,mad_delta,homogeneity" + NAMES
    assert [ln.split(",")[-2:] for ln in a_lines[1:]] == [ln.split(",")[-2:] for ln in s_lines[1:]]
    # the Python formatting path writes the same bytes
    other, other_err = _run(model, pore, raw, bam, tmp_path / "frames.csv", "--border-confidence", str(W), "--parallel-zstd-frames")
    assert other == text and other_err == err
    # without the flag: the same bytes again, and the same compressed file
    again, again_err = _run(model, pore, raw, bam, tmp_path / "again.csv", "--border-confidence", "0")
    assert again == plain and again_err == plain_err
    assert open(tmp_path / "again.csv.zst", "rb").read() == open(tmp_path / "plain.csv.zst", "rb").read()
    assert np.isfinite(res.border_window_probability[:int(res.seg_offsets[-1])]).all()
