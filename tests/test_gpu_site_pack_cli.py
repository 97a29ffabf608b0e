"""GPU (-m gpu): dynamont-resquiggle --site-merge-ranks and --site-table-in on the synthetic POD5 + MAPPED BAM of
tests/test_gpu_site_summary_cli.py (40 reads over two contigs), under torch.distributed.run with two and four ranks, all on
cuda:0, as tests/test_gpu_multirank_cli.py runs them (the payloads through dyn_comm_* over real RCCL where the box connects two
ranks, else torch / gloo). Every rank fills a table of its own; rank 0 merges the packed records by key and writes what one process
writes: the TSV byte for byte, both .npz files array for array, the CSV rows up to order. A sparse table too small for the merged
run ends with exit status 3 and complete positions. A table saved from half of the BAM and given to a run on the other half with
--site-table-in writes the whole BAM's TSV.
No torch in this process (tests/conftest.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, model_for
from dynamont_amd import bam_io, synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from test_gpu_multirank_cli import _exchange
from test_gpu_site_map_cli import HIST, same_table
from test_gpu_site_summary_cli import REFS, _mapping

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


def torchrun(args, port, ranks, started=True):
    """the CLI under torch.distributed.run; returns the finished process (the caller looks at its status). started: the run got
    as far as its process group and names the exchange"""
    exchange = _exchange()
    env = dict(os.environ, DYN_DIST_BACKEND="gloo", DYN_DIST_ONE_DEVICE="1", DYN_DIST_EXCHANGE=exchange, PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr",
           "127.0.0.1", "--master-port", str(port), "-m", "dynamont_amd.segmentation.segment"] + args
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    said = ("exchange: dyn_comm_* (dynamont_amd/csrc/rccl_comm.cpp)" if exchange == "dyn_comm" else "exchange: torch.distributed (gloo)") in r.stderr
    assert said == started, r.stderr[-3000:]
    # (a figure, no pass bar: rank 0's line with the exchange and merge time of this rehearsal on one card, shown with pytest -s)
    print(ranks, "ranks:", *[ln for ln in r.stderr.split("\n") if "site tables merged:" in ln])
    return r


@pytest.fixture(scope="module")
def data(models, tmp_path_factory):
    """the dataset, and ONE process's files with every per-site output on: what the ranks' runs must write"""
    tmp = tmp_path_factory.mktemp("site_pack_cli")
    pore = "rna002"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(6401, 40, pore, mean, sd, (60, 200))
    raw, bam, _ = synth.write_dataset(str(tmp / "in"), "ss", reads, pore, seed=6, container="pod5", basecalls="bam")
    recs = list(bam_io.iter_bam(bam))
    rng = np.random.default_rng(64)
    maps = [_mapping(i, len(r.query_sequence), rng) for i, r in enumerate(recs)]
    rows = [(r.query_name, r.query_sequence, r._tags, m) for r, m in zip(recs, maps)]
    t = lambda name: str(tmp / name)  # noqa: E731
    bam_io.write_bam(t("in/mapped.bam"), rows, references=REFS)
    bam_io.write_bam(t("in/first.bam"), rows[:20], references=REFS)
    bam_io.write_bam(t("in/second.bam"), rows[20:], references=REFS)
    base = lambda b: ["-r", os.path.dirname(raw), "-b", t("in/" + b), "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "7"]  # noqa: E731
    flags = lambda name: ["-o", t(name + ".csv"), "--site-summary", t(name + ".tsv"), "--site-histogram", HIST, "--site-mixture",  # noqa: E731
                          "--site-model-out", t(name + ".model.npz"), "--site-table-out", t(name + ".npz")]
    seg.main(base("mapped.bam") + flags("one") + ["--site-merge-ranks"])       # in one process the flag is accepted and does nothing
    assert len(open(t("one.tsv")).read().split("\n")) > 502
    return base, flags, t


def rows_of(path):
    return zstd_io.decompress(open(path, "rb").read()).decode().splitlines()


def test_two_ranks_dense_write_one_processs_files(data):
    base, flags, t = data
    r = torchrun(base("mapped.bam") + flags("two") + ["--site-merge-ranks"], 29731, 2)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(t("two.tsv"), "rb").read() == open(t("one.tsv"), "rb").read()
    assert same_table(t("two.npz"), t("one.npz")) > 500
    same_table(t("two.model.npz"), t("one.model.npz"))
    one, two = rows_of(t("one.csv.zst")), rows_of(t("two.csv.zst"))
    assert one[0] == two[0] and sorted(one[1:]) == sorted(two[1:]) and len(one) > 500
    said = [ln for ln in r.stderr.split("\n") if "site summary written" in ln]
    single = [ln for ln in open(t("one.tsv")).read().split("\n")]
    assert len(said) == 1 and "%d sites with coverage" % (len(single) - 2) in said[0] and "INCOMPLETE" not in r.stderr
    # the totals and the reads without ids are the sums over the ranks: the line one process prints for the same reads
    with np.load(t("two.npz")) as z:
        assert "reads_ok %d, rows_added %d," % (int(z["totals"][0]), int(z["totals"][1])) in said[0]
    # without the flag the ranks are refused as before, with the flag named
    r = torchrun(base("mapped.bam") + ["-o", t("refused.csv"), "--site-summary", t("refused.tsv")], 29732, 2, started=False)
    assert r.returncode != 0 and "--site-summary runs in one process: merging the per-site tables of several ranks is not built yet" in r.stderr
    assert not os.path.exists(t("refused.tsv"))


def test_four_ranks_sparse_write_the_same_tsv(data):
    base, flags, t = data
    r = torchrun(base("mapped.bam") + flags("four") + ["--site-merge-ranks", "--site-capacity", "4096"], 29734, 4)
    assert r.returncode == 0, r.stderr[-3000:]
    assert open(t("four.tsv"), "rb").read() == open(t("one.tsv"), "rb").read()
    assert same_table(t("four.npz"), t("one.npz")) > 500
    assert "rows dropped on the ranks 0, records dropped in the merge 0" in r.stderr and "INCOMPLETE" not in r.stderr


def test_two_ranks_whose_merge_drops_end_with_status_3_and_complete_positions(data):
    """--site-capacity 900 holds either rank's positions (the even reads lie on one contig, the odd ones on the other: 650 and 445 of
    them) and not their union: the ranks drop nothing, rank 0's merge does"""
    base, flags, t = data
    r = torchrun(base("mapped.bam") + ["-o", t("drop.csv"), "--site-summary", t("drop.tsv"), "--site-histogram", HIST, "--site-merge-ranks",
                                       "--site-capacity", "900"], 29736, 2)
    assert r.returncode != 0
    assert "exitcode  : 3" in r.stderr or "exitcode: 3" in r.stderr, r.stderr[-3000:]
    said = [ln for ln in r.stderr.split("\n") if "INCOMPLETE" in ln]
    assert len(said) == 1 and "larger --site-capacity" in said[0] and "900" in said[0], r.stderr[-3000:]
    dropped = int(said[0].split("INCOMPLETE: ")[1].split(" ")[0])
    assert "rows dropped on the ranks 0, records dropped in the merge %d" % dropped in r.stderr and dropped > 0
    small, full = open(t("drop.tsv")).read().split("\n"), open(t("one.tsv")).read().split("\n")
    cut = lambda ln: "\t".join(ln.split("\t")[:len(small[0].split("\t"))])  # noqa: E731  (the fixture's run also has the mixture columns)
    assert small[0] == cut(full[0]) and 0 < len(small) - 2 <= 900 and len(small) + dropped == len(full)
    whole = [cut(ln) for ln in full]
    assert set(small[1:-1]) <= set(whole[1:-1])                          # every position in it is complete: its line of the whole run
    pos = [whole.index(ln) for ln in small[1:-1]]
    assert pos == sorted(pos)                                            # in reference order


def test_table_in_adds_an_earlier_runs_table(data, capfd):
    """the first 20 reads saved with --site-table-out, the other 20 run with --site-table-in: the TSV and the table of the whole BAM"""
    base, flags, t = data
    seg.main(base("first.bam") + ["-o", t("first.csv"), "--site-summary", t("first.tsv"), "--site-histogram", HIST, "--site-table-out", t("first.npz")])
    capfd.readouterr()
    seg.main(base("second.bam") + flags("both") + ["--site-table-in", t("first.npz")])
    err = capfd.readouterr().err
    assert open(t("both.tsv"), "rb").read() == open(t("one.tsv"), "rb").read()
    assert same_table(t("both.npz"), t("one.npz")) > 500
    with np.load(t("first.npz")) as z:
        assert "site table in: %s: %d sites with coverage added" % (t("first.npz"), z["site"].size) in err
    # a sparse run takes it the same way
    seg.main(base("second.bam") + ["-o", t("both_s.csv"), "--site-summary", t("both_s.tsv"), "--site-histogram", HIST, "--site-mixture",
                                   "--site-table-in", t("first.npz"), "--site-capacity", "4096"])
    assert open(t("both_s.tsv"), "rb").read() == open(t("one.tsv"), "rb").read()
    with pytest.raises(ValueError, match=r"--site-table-in .*first.npz: its histograms \(32 bins"):
        seg.main(base("second.bam") + ["-o", t("no.csv"), "--site-summary", t("no.tsv"), "--site-histogram", "16:-4:4", "--site-table-in", t("first.npz")])
    assert not os.path.exists(t("no.tsv"))
