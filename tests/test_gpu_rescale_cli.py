"""GPU (-m gpu): dynamont-resquiggle --rescale-iters. With N > 0 the CLI writes, read for read, the rows the Python path
formats for the same normalised signals aligned with Aligner.set_rescale(N); --rescale-iters 0 writes the bytes of a run
without the flag."""
import os

import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import Aligner, synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel, segmentation_to_string

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

PORE = "rna004"


def _run(model, raw, bam, out, *extra):
    seg.main(["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", PORE, "--model_path", model,
              "--batch-reads", "4", "-o", str(out)] + list(extra))
    return open(str(out) + ".zst", "rb").read()


def test_rescale_iters_rows_and_off_bytes(models, tmp_path):
    model = model_for(models, PORE)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(5201, 14, PORE, mean, sd, (60, 220))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "rs", reads, PORE, seed=3, sm=95.0, sd=14.0)
    plain = _run(model, raw, bam, tmp_path / "plain.csv")
    off = _run(model, raw, bam, tmp_path / "off.csv", "--rescale-iters", "0")
    assert off == plain
    text = zstd_io.decompress(_run(model, raw, bam, tmp_path / "rs.csv", "--rescale-iters", "2")).decode()
    lines = text.splitlines(keepends=True)
    assert lines[0] == seg.CSV_HEADER.decode()
    rows = {}
    for ln in lines[1:]:
        rows.setdefault(ln.split(",", 1)[0], []).append(ln)
    assert len(rows) == len(reads)
    al = Aligner(model, PORE, device=0)
    al.set_rescale(2)
    for rid, got in rows.items():
        x, s = expected[int(rid.rsplit("-", 1)[1])]
        x = x.copy()
        hampel(x)   # the CLI aligns the Hampel-filtered signal (segment.py:146-153)
        f = got[0].split(",")
        s0 = int(f[2])
        res = al.align_batch([x], [s], True)
        assert res.rescale_iters[0] >= 1
        want = segmentation_to_string(res.read(0), f[0], f[1], s0, s0 + len(x), s, 9, True)
        assert "".join(got).encode() == want, rid
    al.close()
