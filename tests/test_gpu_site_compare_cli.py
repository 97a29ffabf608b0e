"""GPU (-m gpu): dynamont-resquiggle --site-table-out TABLE.npz and --site-control TABLE.npz on two synthetic POD5 + MAPPED BAM
datasets over the references of tests/test_gpu_site_summary_cli.py (40 reads each, built the same way). Run A saves its table; run
B compares itself against it. B's eight new columns must equal the restatement (tests/site_compare_cases.py) over the two saved
tables, Aligner.site_compare of an in-process table that holds both samples, and site_welch of their rows; B's other columns and
its .csv are those of a run without --site-control; A's TSV is that of a run without --site-table-out, byte for byte.
No torch in this process (tests/conftest.py)."""
import os

import numpy as np
import pytest

import site_compare_cases as scc
from conftest import model_for
from dynamont_amd import Aligner, bam_io, synth
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation import utils
from dynamont_amd.sites import contig_offsets
from test_gpu_site_summary_cli import REFS, _mapping

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

SPEC = (32, -4.0, 4.0)


def dataset(tmp_path, name, pore, model, seed):
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(seed, 40, pore, mean, sd, (60, 200))
    raw, bam, _ = synth.write_dataset(str(tmp_path / name), name, reads, pore, seed=seed % 97, container="pod5", basecalls="bam")
    recs = list(bam_io.iter_bam(bam))
    rng = np.random.default_rng(64)                                  # the same mapping draws: the two samples cover the same regions
    maps = [_mapping(i, len(r.query_sequence), rng) for i, r in enumerate(recs)]
    mapped = str(tmp_path / name / "mapped.bam")
    bam_io.write_bam(mapped, [(r.query_name, r.query_sequence, r._tags, m) for r, m in zip(recs, maps)], references=REFS)
    return ["-r", os.path.dirname(raw), "-b", mapped, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "7"]


def dense(table, n):
    """the saved sparse columns as full-length lists of Python ints"""
    site = table["site"].astype(np.int64)
    out = {k: [0] * n for k in ("n_rows", "M1", "M2")}
    level, dwell = [[0] * (SPEC[0] + 2) for _ in range(n)], [[0] * 16 for _ in range(n)]
    for j, s in enumerate(site.tolist()):
        for k in out:
            out[k][s] = int(table[k][j])
        level[s], dwell[s] = table["level"][j].tolist(), table["dwell"][j].tolist()
    return out, level, dwell


def test_a_run_against_a_saved_control(models, tmp_path, capfd):
    pore = "rna002"
    model = model_for(models, pore)
    base_a, base_b = dataset(tmp_path, "ctl", pore, model, 6401), dataset(tmp_path, "run", pore, model, 6402)
    f = lambda name: str(tmp_path / name)  # noqa: E731
    hist = ["--site-histogram", "32:-4:4"]
    seg.main(base_a + ["-o", f("a.csv"), "--site-summary", f("a.tsv"), "--site-table-out", f("a.npz")] + hist)
    seg.main(base_a + ["-o", f("a0.csv"), "--site-summary", f("a0.tsv")] + hist)
    assert open(f("a.tsv"), "rb").read() == open(f("a0.tsv"), "rb").read()
    assert open(f("a.csv.zst"), "rb").read() == open(f("a0.csv.zst"), "rb").read()
    capfd.readouterr()
    seg.main(base_b + ["-o", f("b.csv"), "--site-summary", f("b.tsv"), "--site-control", f("a.npz"), "--site-table-out", f("b.npz")] + hist)
    err = capfd.readouterr().err
    seg.main(base_b + ["-o", f("b0.csv"), "--site-summary", f("b0.tsv"), "--site-table-out", f("b0.npz")] + hist)
    assert open(f("b.csv.zst"), "rb").read() == open(f("b0.csv.zst"), "rb").read()
    ta, tb, tb0 = (utils.load_site_table(f(n)) for n in ("a.npz", "b.npz", "b0.npz"))
    assert "site control: %s: %d sites with coverage loaded" % (f("a.npz"), ta["site"].size) in err
    # --site-table-out beside --site-control saves the run's half only: what the run without a control saves
    with np.load(f("b.npz")) as z, np.load(f("b0.npz")) as z0:
        assert sorted(z.files) == sorted(z0.files) and all(z[k].tobytes() == z0[k].tobytes() for k in z.files)
    n = sum(ln for _, ln in REFS)
    assert ta["num_sites"] == tb["num_sites"] == n and ta["hist_spec"] == SPEC and ta["ref_names"] == [r for r, _ in REFS]
    assert ta["site"].size > 400 and tb["site"].size > 400 and np.intersect1d(ta["site"], tb["site"]).size > 300
    # the restatement over the two saved tables: A of the comparison is the RUN (b), B the control (a)
    run, run_lv, run_dw = dense(tb, n)
    ctl, ctl_lv, ctl_dw = dense(ta, n)
    want = scc.compare_arrays(run_lv + ctl_lv, run_dw + ctl_dw, 0, n, n)
    # ... and the GPU's comparison of an in-process table that holds both
    al = Aligner(model, pore, device=0)
    al.set_site_summary(2 * n)
    al.set_site_histogram(*SPEC)
    assert utils.load_site_control(al, tb, 0) == tb["site"].size and utils.load_site_control(al, ta, n) == ta["site"].size
    got = al.site_compare(0, n)
    for k in scc.COLUMNS:
        assert np.array_equal(got[k], want[k]), k
    al.close()
    offs = contig_offsets([ln for _, ln in REFS])
    names = [r for r, _ in REFS]
    lines, plain = open(f("b.tsv")).read().split("\n"), open(f("b0.tsv")).read().split("\n")
    assert lines[0] == plain[0] + "\t" + utils.SITE_CONTROL_HEADER and len(lines) == len(plain) and lines[-1] == ""
    assert len(lines) - 2 == tb["site"].size
    both = 0
    for ln, pl in zip(lines[1:-1], plain[1:-1]):
        p = ln.split("\t")
        assert len(p) == 19 and p[:11] == pl.split("\t")              # B's other columns: the run without --site-control
        s = int(offs[names.index(p[0])]) + int(p[1]) - 1
        n_a, n_b, num = int(want["n_a"][s]), int(want["n_b"][s]), int(want["level_num"][s])
        assert n_a == int(p[2]) > 0 and n_b == ctl["n_rows"][s]
        d = float(num) / (float(n_a) * float(n_b)) if n_b else float("nan")
        dd = float(int(want["dwell_num"][s])) / (float(n_a) * float(n_b)) if n_b else float("nan")
        at = int(want["level_at"][s])
        edge = float("nan") if at == scc.NO_AT else (float("inf") if at == SPEC[0] + 1 else SPEC[1] + at * 0.25)
        t, df = utils.site_welch((run["n_rows"][s], run["M1"][s], run["M2"][s]), (ctl["n_rows"][s], ctl["M1"][s], ctl["M2"][s]))
        assert p[11:] == [str(n_b), repr(d), repr(utils.ks_two_sample_p(d, n_a, n_b)), repr(edge), str(int(want["level_side"][s])), repr(dd),
                          repr(t), repr(df)], (p[0], p[1], p[11:])
        both += n_b > 0
    assert both > 300
