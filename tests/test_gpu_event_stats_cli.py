"""GPU (-m gpu): dynamont-resquiggle --event-stats. The first ten columns and `.errors` are those of a run without the flag;
the three new columns are the restated levels (tests/test_gpu_event_stats.py) formatted by Python; every output path of the
CLI (native sink over read-by-read jobs and over BAM columns, --host-preprocess, --parallel-zstd-frames, two ranks) writes
the same bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, model_for
from dynamont_amd import synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel
from test_gpu_event_stats import levels_of

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

PORE = "rna004"


def _dataset(models, tmp_path, basecalls):
    model = model_for(models, PORE)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(5101, 14, PORE, mean, sd, (60, 220))
    raw, bam, expected = synth.write_dataset(str(tmp_path / f"in_{basecalls}"), "ev", reads, PORE, seed=3, basecalls=basecalls)
    if basecalls == "tsv":   # one read that fails in the aligner: its .errors line must not change
        lines = open(bam).read().splitlines()
        f = lines[4].split("\t"); f[1] = f[1][:30] + "N" + f[1][31:]; lines[4] = "\t".join(f)
        open(bam, "w").write("\n".join(lines) + "\n")
    return model, raw, bam, expected


def _run(model, raw, bam, out, *extra):
    seg.main(["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", PORE, "--model_path", model,
              "--batch-reads", "4", "-o", str(out)] + list(extra))
    text = zstd_io.decompress(open(str(out) + ".zst", "rb").read()).decode()
    errors = open(os.path.splitext(str(out))[0] + ".errors").read() if os.path.exists(os.path.splitext(str(out))[0] + ".errors") else ""
    return text, errors


def test_event_columns_and_every_cli_path(models, tmp_path):
    model, raw, bam, expected = _dataset(models, tmp_path, "tsv")
    plain, plain_err = _run(model, raw, bam, tmp_path / "plain.csv")
    ev, ev_err = _run(model, raw, bam, tmp_path / "ev.csv", "--event-stats")
    assert ev_err == plain_err and plain_err.count("\n") >= 1
    p_lines, e_lines = plain.splitlines(), ev.splitlines()
    assert e_lines[0] == p_lines[0] + ",level_mean,level_stdv,level_median"
    assert len(p_lines) == len(e_lines) > 300
    rows = {}
    for p, e in zip(p_lines[1:], e_lines[1:]):
        f = e.split(",")
        assert ",".join(f[:10]) == p
        rows.setdefault(f[0], []).append(f)
    # the levels: the restatement over the normalised signal the harness reconstructs, formatted as Python formats them
    for rid, fs in rows.items():
        x = expected[int(rid.rsplit("-", 1)[1])][0].copy()
        hampel(x)   # the CLI aligns the Hampel-filtered signal (segment.py:146-153)
        s0 = int(fs[0][2])
        assert int(fs[-1][3]) - s0 == len(x)
        lv = levels_of(x, [int(f[2]) - s0 for f in fs])
        for j, f in enumerate(fs):
            assert f[10:] == [f"{lv[0, j]:.6f}", f"{lv[1, j]:.6f}", f"{lv[2, j]:.6f}"], (rid, j)
    # every other path: the same file bytes
    for tag, extra in (("host", ["--host-preprocess"]), ("frames", ["--parallel-zstd-frames"])):
        text, err = _run(model, raw, bam, tmp_path / f"{tag}.csv", "--event-stats", *extra)
        assert text == ev and err == ev_err, tag
    env = dict(os.environ, DYN_DIST_BACKEND="gloo", DYN_DIST_ONE_DEVICE="1", DYN_DIST_EXCHANGE="torch", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29641", "-m", "dynamont_amd.segmentation.segment", "-r", os.path.dirname(raw), "-b", bam, "--mode",
           "basic", "-p", PORE, "--model_path", model, "--batch-reads", "4", "-o", str(tmp_path / "ranks.csv"), "--event-stats"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    multi = zstd_io.decompress(open(tmp_path / "ranks.csv.zst", "rb").read()).decode().splitlines()
    assert multi[0] == e_lines[0] and sorted(multi[1:]) == sorted(e_lines[1:])


def test_bam_columns_front_end(models, tmp_path):
    model, raw, bam, expected = _dataset(models, tmp_path, "bam")
    col, col_err = _run(model, raw, bam, tmp_path / "col.csv", "--event-stats")
    host, host_err = _run(model, raw, bam, tmp_path / "host.csv", "--event-stats", "--host-preprocess")
    plain, _ = _run(model, raw, bam, tmp_path / "plain.csv")
    assert col == host and col_err == host_err
    assert [",".join(l.split(",")[:10]) for l in col.splitlines()[1:]] == plain.splitlines()[1:]
