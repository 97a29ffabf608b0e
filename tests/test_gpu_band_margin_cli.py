"""GPU (-m gpu): dynamont-resquiggle --band-report FILE. One line per read with the integers the API returns for the same read
(Aligner.set_band_margin over the normalised, Hampel-filtered signal), the same bytes from one process and from two ranks, and
a CSV that does not know about the flag: its bytes are those of a run without it."""
import os

import numpy as np
import pytest

import band_margin_cases as bmc
from conftest import model_for
from dynamont_amd import Aligner, synth
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


def test_band_report_one_process_two_ranks_and_the_api(models, tmp_path):
    from test_gpu_multirank_cli import _torchrun
    pore, band = "rna002", 50
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(7301, 11, pore, mean, sd, (60, 200))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "bm", reads, pore, seed=6, container="pod5", basecalls="bam")
    base = ["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "3",
            "--band", str(band)]
    seg.main(base + ["-o", str(tmp_path / "plain.csv")])
    seg.main(base + ["-o", str(tmp_path / "one.csv"), "--band-report", str(tmp_path / "one.tsv")])
    # the CSV is byte-equal with and without the flag
    assert open(tmp_path / "one.csv.zst", "rb").read() == open(tmp_path / "plain.csv.zst", "rb").read()
    one = open(tmp_path / "one.tsv", "rb").read()
    lines = one.decode().split("\n")
    assert lines[0] + "\n" == seg.BAND_REPORT_HEADER.decode() and lines[-1] == "" and len(lines) == len(reads) + 2
    assert lines[1:-1] == sorted(lines[1:-1])
    # the API on the signals the CLI aligns (normalised, Hampel-filtered) and the sequences it hands the aligner
    sig, seq = [], []
    for x, s in expected:
        x = x.copy()
        hampel(x)
        sig.append(x)
        seq.append(s)
    al = Aligner(model, pore, band=band, device=0)
    al.set_band_margin(True)
    res = al.align_batch(sig, seq, True)
    assert (res.status == 0).all()
    want = np.stack([res.band_margin_low, res.band_margin_high, res.band_edge_rows])
    assert np.array_equal(want, np.array([bmc.margins_of_result(res, i, len(sig[i]) + 1, band) for i in range(res.n)], dtype=np.uint32).T)
    al.close()
    by_values = sorted("\t".join(ln.split("\t")[1:]) for ln in lines[1:-1])
    api = seg.band_report_lines([""] * res.n, [len(x) + 1 for x in sig], [int(n) + 1 for n in res.n_segments], band, *want)
    assert by_values == sorted(ln[1:] for ln in api)
    assert (np.minimum(want[0], want[1]) != bmc.NONE).any()                          # the report carries information
    # Python formatting path (rank-0 listener): the same report
    seg.main(base + ["-o", str(tmp_path / "frames.csv"), "--band-report", str(tmp_path / "frames.tsv"), "--parallel-zstd-frames"])
    assert open(tmp_path / "frames.tsv", "rb").read() == one
    # two ranks: the same bytes
    _torchrun("dynamont_amd.segmentation.segment", base + ["-o", str(tmp_path / "two.csv"), "--band-report", str(tmp_path / "two.tsv")], 29661)
    assert open(tmp_path / "two.tsv", "rb").read() == one
