"""GPU (-m gpu): dynamont-resquiggle --site-mixture [MAX_ITERS] on the two synthetic POD5 + MAPPED BAM datasets of
tests/test_gpu_site_compare_cli.py (a control and a run, 40 reads each, built the same way). Without the flag the --site-summary
file and the .csv are those of a run that never heard of it; with it, the file's other columns stay byte for byte and the seven
added columns equal utils.site_mixture_columns over Aligner.site_mixture of an in-process table loaded from the run's saved table;
with --site-control beside it the eleven added columns equal the pooled fit of a table that holds both samples. The refusals.
No torch in this process (tests/conftest.py)."""
import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import Aligner
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation import utils
from dynamont_amd.sites import contig_offsets
from test_gpu_site_compare_cli import SPEC, dataset
from test_gpu_site_summary_cli import REFS

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


def test_the_mixture_columns_of_a_run_and_of_a_run_against_a_control(models, tmp_path):
    pore = "rna002"
    model = model_for(models, pore)
    base_a, base_b = dataset(tmp_path, "ctl", pore, model, 6401), dataset(tmp_path, "run", pore, model, 6402)
    f = lambda name: str(tmp_path / name)  # noqa: E731
    hist = ["--site-histogram", "32:-4:4"]
    seg.main(base_a + ["-o", f("a.csv"), "--site-summary", f("a.tsv"), "--site-table-out", f("a.npz")] + hist)
    seg.main(base_b + ["-o", f("b0.csv"), "--site-summary", f("b0.tsv"), "--site-table-out", f("b0.npz")] + hist)
    seg.main(base_b + ["-o", f("b1.csv"), "--site-summary", f("b1.tsv")] + hist + ["--site-mixture"])
    seg.main(base_b + ["-o", f("b2.csv"), "--site-summary", f("b2.tsv"), "--site-control", f("a.npz"), "--site-mixture", "40"] + hist)
    seg.main(base_b + ["-o", f("b3.csv"), "--site-summary", f("b3.tsv"), "--site-control", f("a.npz")] + hist)
    for name in ("b1", "b2", "b3"):
        assert open(f(name + ".csv.zst"), "rb").read() == open(f("b0.csv.zst"), "rb").read()
    ta, tb = utils.load_site_table(f("a.npz")), utils.load_site_table(f("b0.npz"))
    n = sum(ln for _, ln in REFS)
    offs = contig_offsets([ln for _, ln in REFS])
    names = [r for r, _ in REFS]
    site_of = lambda p: int(offs[names.index(p[0])]) + int(p[1]) - 1  # noqa: E731
    # the run alone
    al = Aligner(model, pore, device=0)
    al.set_site_summary(n)
    al.set_site_histogram(*SPEC)
    assert utils.load_site_control(al, tb, 0) == tb["site"].size
    alone = al.site_mixture(0, n)
    want = utils.site_mixture_columns(alone)
    al.close()
    lines, plain = open(f("b1.tsv")).read().split("\n"), open(f("b0.tsv")).read().split("\n")
    assert lines[0] == plain[0] + "\t" + utils.SITE_MIXTURE_HEADER and len(lines) == len(plain) == tb["site"].size + 2
    fitted = 0                                                            # (40 reads over a thousand sites: few reach min_n = 8 rows)
    for ln, pl in zip(lines[1:-1], plain[1:-1]):
        assert ln.startswith(pl + "\t")                                   # the other columns: the run without the flag, byte for byte
        p = ln.split("\t")
        assert len(p) == 11 + 7 and "\t".join(p[11:]) == want[site_of(p)], (p[0], p[1])
        fitted += p[-1] != "1"
    assert fitted > 20 and (alone["status"] == 1).sum() > 0 and "nan\tnan\tnan\tnan\tnan\t0\t1" in want
    # the run pooled with its control: A the run, B the control
    al = Aligner(model, pore, device=0)
    al.set_site_summary(2 * n)
    al.set_site_histogram(*SPEC)
    assert utils.load_site_control(al, tb, 0) == tb["site"].size and utils.load_site_control(al, ta, n) == ta["site"].size
    pooled = al.site_mixture(0, n, n, max_iters=40)
    want = utils.site_mixture_columns(pooled, True)
    al.close()
    lines, plain = open(f("b2.tsv")).read().split("\n"), open(f("b3.tsv")).read().split("\n")
    assert lines[0] == plain[0] + "\t" + utils.SITE_MIXTURE_HEADER + "\t" + utils.SITE_MIXTURE_CONTROL_HEADER and len(lines) == len(plain)
    both = 0
    for ln, pl in zip(lines[1:-1], plain[1:-1]):
        assert ln.startswith(pl + "\t")
        p = ln.split("\t")
        s = site_of(p)
        assert len(p) == 19 + 11 and "\t".join(p[19:]) == want[s], (p[0], p[1])
        if pooled["n_b"][s] and pooled["n_a"][s] and pooled["status"][s] != 1:
            both += 1
            assert float(p[27]) == float(p[19]) - float(p[26]) and 0.0 <= float(p[29]) <= 1.0
    assert both > 20 and int(pooled["iters"].max()) <= 40


def test_refusals(models, tmp_path):
    pore = "rna002"
    model = model_for(models, pore)
    base = ["-r", str(tmp_path), "-b", str(tmp_path / "none.bam"), "--mode", "basic", "-p", pore, "--model_path", model, "-o", str(tmp_path / "x.csv")]
    with pytest.raises(ValueError, match=r"--site-mixture fits the per-site histograms of the run: it needs --site-summary FILE and --site-histogram"):
        seg.main(base + ["--site-mixture"])
    with pytest.raises(ValueError, match=r"--site-mixture fits the per-site histograms of the run: it needs --site-summary FILE and --site-histogram"):
        seg.main(base + ["--site-summary", str(tmp_path / "x.tsv"), "--site-mixture", "12"])
    with pytest.raises(ValueError, match=r"--site-mixture 2000: MAX_ITERS must be 1 \.\. 1024"):
        seg.main(base + ["--site-summary", str(tmp_path / "x.tsv"), "--site-histogram", "32:-4:4", "--site-mixture", "2000"])
    assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "x.csv.zst").exists()
