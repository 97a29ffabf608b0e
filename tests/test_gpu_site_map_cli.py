"""GPU (-m gpu): dynamont-resquiggle --site-capacity on the synthetic POD5 + MAPPED BAM of tests/test_gpu_site_summary_cli.py (40
reads over two contigs). With room for every site the sparse run writes the dense run's TSV byte for byte and the dense run's
table (every member of the .npz bit for bit; the zip container itself carries the time it was written) -- with --site-histogram,
--site-control and --site-mixture on; the .csv is byte-equal to a run without any site flag. A capacity too small for the fixture
still writes a TSV whose every line is the dense run's line for that site, says so on stderr and ends with exit status 3; a
control that does not fit such a table ends the run with a MemoryError that names the flag.
No torch in this process (tests/conftest.py)."""
import os

import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import bam_io, synth
from dynamont_amd.segmentation import segment as seg
from test_gpu_site_summary_cli import REFS, _mapping

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

HIST = "32:-4:4"


def same_table(a, b):
    with np.load(a) as x, np.load(b) as y:
        assert sorted(x.files) == sorted(y.files)
        for k in x.files:
            assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape and x[k].tobytes() == y[k].tobytes(), k
        return int(x["site"].size)


def test_sparse_run_writes_the_dense_runs_files_and_a_full_table_says_so(models, tmp_path, capfd):
    pore = "rna002"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(6401, 40, pore, mean, sd, (60, 200))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "ss", reads, pore, seed=6, container="pod5", basecalls="bam")
    recs = list(bam_io.iter_bam(bam))
    rng = np.random.default_rng(64)
    maps = [_mapping(i, len(r.query_sequence), rng) for i, r in enumerate(recs)]
    mapped = str(tmp_path / "in" / "mapped.bam")
    bam_io.write_bam(mapped, [(r.query_name, r.query_sequence, r._tags, m) for r, m in zip(recs, maps)], references=REFS)
    base = ["-r", os.path.dirname(raw), "-b", mapped, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "7"]
    t = lambda name: str(tmp_path / name)  # noqa: E731
    csv = lambda name: open(t(name + ".csv.zst"), "rb").read()  # noqa: E731

    with pytest.raises(ValueError, match="--site-capacity sizes the sparse per-site table: it needs --site-summary"):
        seg.main(base + ["-o", t("refused.csv"), "--site-capacity", "100"])
    with pytest.raises(ValueError, match="ROWS must be 1 .. 4294967294"):
        seg.main(base + ["-o", t("refused.csv"), "--site-summary", t("refused.tsv"), "--site-capacity", "4294967295"])
    assert not os.path.exists(t("refused.csv.zst")) and not os.path.exists(t("refused.tsv"))     # before anything starts

    seg.main(base + ["-o", t("plain.csv")])
    # the control: the same reads, one table each way
    seg.main(base + ["-o", t("c_dense.csv"), "--site-summary", t("c_dense.tsv"), "--site-histogram", HIST, "--site-table-out", t("c_dense.npz")])
    capfd.readouterr()
    seg.main(base + ["-o", t("c_sparse.csv"), "--site-summary", t("c_sparse.tsv"), "--site-histogram", HIST, "--site-table-out", t("c_sparse.npz"),
                     "--site-capacity", "4096"])
    err = capfd.readouterr().err
    covered = same_table(t("c_sparse.npz"), t("c_dense.npz"))
    assert covered > 500 and "sparse table: %d of 4096 rows taken, rows_dropped 0" % covered in err and "INCOMPLETE" not in err
    dense_tsv = open(t("c_dense.tsv")).read()
    assert open(t("c_sparse.tsv")).read() == dense_tsv and len(dense_tsv.split("\n")) == covered + 2
    # the run against the control, every site column on
    flags = ["--site-histogram", HIST, "--site-control", t("c_dense.npz"), "--site-mixture", "--site-table-out"]
    seg.main(base + ["-o", t("dense.csv"), "--site-summary", t("dense.tsv")] + flags + [t("dense.npz")])
    seg.main(base + ["-o", t("sparse.csv"), "--site-summary", t("sparse.tsv")] + flags + [t("sparse.npz"), "--site-capacity", "8192"])
    assert open(t("sparse.tsv")).read() == open(t("dense.tsv")).read()
    assert "mix_lor" in open(t("dense.tsv")).readline() and "ks_d" in open(t("dense.tsv")).readline()
    assert same_table(t("sparse.npz"), t("dense.npz")) == covered
    for name in ("c_dense", "c_sparse", "dense", "sparse"):
        assert csv(name) == csv("plain"), name                       # no site flag changes a byte of the rows
    # a table too small for the fixture: complete sites, missing sites, one line that says so, exit status 3
    capfd.readouterr()
    with pytest.raises(SystemExit) as stop:
        seg.main(base + ["-o", t("small.csv"), "--site-summary", t("small.tsv"), "--site-histogram", HIST, "--site-capacity", "300"])
    assert stop.value.code == 3
    err = capfd.readouterr().err
    said = [ln for ln in err.split("\n") if "INCOMPLETE" in ln]
    assert len(said) == 1 and "larger --site-capacity" in said[0] and "300" in said[0]
    dropped = int(said[0].split("INCOMPLETE: ")[1].split(" ")[0])
    assert dropped > 0 and "rows_dropped %d" % dropped in err
    small, full = open(t("small.tsv")).read().split("\n"), dense_tsv.split("\n")
    assert small[0] == full[0] and 0 < len(small) - 2 <= 300 and len(small) < len(full)
    assert set(small[1:-1]) <= set(full[1:-1])                       # every site in it equals its dense line
    pos = [full.index(ln) for ln in small[1:-1]]
    assert pos == sorted(pos)                                        # in reference order
    assert csv("small") == csv("plain")
    # a control that does not fit beside the run: refused with the flag's name before any read is aligned, no TSV
    with pytest.raises(MemoryError, match=r"--site-capacity 300: the control .*c_dense.npz does not fit the sparse table beside the run "
                                          r"\(.*sites found no bucket.*the other sites were added\); run again with a larger --site-capacity"):
        seg.main(base + ["-o", t("nofit.csv"), "--site-summary", t("nofit.tsv")] + flags + [t("nofit.npz"), "--site-capacity", "300"])
    assert not os.path.exists(t("nofit.tsv")) and not os.path.exists(t("nofit.npz"))
