"""GPU (-m gpu): dynamont-resquiggle --site-mixture --site-model-out MODEL.npz, then --site-model MODEL.npz on a later run, over the
synthetic POD5 + MAPPED BAM dataset of tests/test_gpu_site_summary_cli.py (40 reads over two contigs). The later run's .csv gains
site_probability,site_z on every row: the two columns equal the Python API's on the same reads (the model file uploaded onto a
handle of the test's own, the reads aligned in one batch), every other column equals a run without --site-model byte for byte, a
model fitted over other contigs is refused with its message, and a --site-capacity too small for the model reports the dropped rows.
No torch in this process (tests/conftest.py)."""
import os

import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import Aligner, bam_io, synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation import utils
from dynamont_amd.sites import DYN_SITE_NONE, contig_offsets, site_ids_from_cigar, to_aligner_orientation
from test_gpu_site_summary_cli import REFS, _mapping

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


def rows_of(path):
    lines = zstd_io.decompress(open(path, "rb").read()).decode().split("\n")
    assert lines[-1] == ""
    return lines[0], lines[1:-1]


def test_a_saved_model_scores_the_rows_of_a_later_run(models, tmp_path, capfd):
    pore = "rna002"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(6401, 40, pore, mean, sd, (60, 200))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "sc", reads, pore, seed=6, container="pod5", basecalls="bam")
    recs = list(bam_io.iter_bam(bam))
    rng = np.random.default_rng(64)
    maps = [_mapping(i, len(r.query_sequence), rng) for i, r in enumerate(recs)]
    mapped = str(tmp_path / "in" / "mapped.bam")
    bam_io.write_bam(mapped, [(r.query_name, r.query_sequence, r._tags, m) for r, m in zip(recs, maps)], references=REFS)
    base = ["-r", os.path.dirname(raw), "-b", mapped, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "7"]
    f = lambda name: str(tmp_path / name)  # noqa: E731
    hist = ["--site-histogram", "32:-4:4"]
    seg.main(base + ["-o", f("fit.csv"), "--site-summary", f("fit.tsv"), "--site-mixture", "--site-model-out", f("model.npz")] + hist)
    err = capfd.readouterr().err
    saved = utils.load_site_model(f("model.npz"), [r for r, _ in REFS], [ln for _, ln in REFS])
    n_sites = sum(ln for _, ln in REFS)
    assert saved["site"].size > 8 and saved["num_sites"] == n_sites and saved["histogram"] == (32, -4.0, 4.0)
    assert "site model written: %s: %d positions with a fitted model" % (f("model.npz"), saved["site"].size) in err
    seg.main(base + ["-o", f("called.csv"), "--site-summary", f("called.tsv"), "--site-model", f("model.npz")])
    err = capfd.readouterr().err
    assert "site model: %s: %d positions loaded\n" % (f("model.npz"), saved["site"].size) in err
    seg.main(base + ["-o", f("plain.csv"), "--site-summary", f("plain.tsv")])
    assert open(f("called.tsv"), "rb").read() == open(f("plain.tsv"), "rb").read()
    # every other column: the run without --site-model, byte for byte
    (h1, called), (h0, plain) = rows_of(f("called.csv.zst")), rows_of(f("plain.csv.zst"))
    assert h1 == h0 + ",site_probability,site_z" and len(called) == len(plain) > 1000
    assert all(c.startswith(p + ",") and c[len(p) + 1:].count(",") == 1 for c, p in zip(called, plain))
    by_read = {}
    for c, p in zip(called, plain):
        by_read.setdefault(c.split(",")[0], []).append(c[len(p) + 1:])
    # the Python API on the same reads: the signal the pipeline aligned, the ids of the BAM's mapping, the model file uploaded
    offs = contig_offsets([ln for _, ln in REFS])
    sigs, seqs, ids = [], [], []
    for rec, (flag, ref, pos, cigar), (x, seq) in zip(recs, maps, expected):
        x = x.copy()
        utils.hampel(x)
        l_seq, L = len(rec.query_sequence), len(seq)
        placeholder = len(cigar) == 2 and cigar[1] & 0xF == 3
        if flag & (4 | 16 | 256 | 2048) or placeholder:
            ids.append(np.full(L, DYN_SITE_NONE, dtype=np.uint32))
        else:
            ids.append(to_aligner_orientation(site_ids_from_cigar(pos, cigar, l_seq, offs[ref]), True, L - l_seq))
        sigs.append(x)
        seqs.append(seq)
    al = Aligner(model, pore, device=0)
    al.set_site_summary(n_sites)
    assert utils.upload_site_model(al, saved) == {"stored": saved["site"].size, "dropped": 0}
    al.set_site_calls(True)
    res = al.align_batch(sigs, seqs, True, site_ids=np.concatenate(ids))
    al.close()
    fmt = lambda v: "nan" if v != v else "%.6f" % v  # noqa: E731
    checked = with_call = 0
    for i, rec in enumerate(recs):
        if rec.query_name not in by_read:
            continue
        assert res.status[i] == 0
        a, nseg = int(res.seg_offsets[i]), int(res.n_segments[i])
        want = ["%s,%s" % (fmt(float(p)), fmt(float(z))) for p, z in zip(res.site_probability[a:a + nseg], res.site_z[a:a + nseg])]
        assert by_read[rec.query_name] == want, rec.query_name
        checked += 1
        with_call += sum(not w.endswith("nan") for w in want)
    assert checked == len(by_read) >= 36 and with_call > 50
    # a model fitted over other contigs: refused before anything is started
    other = {k: saved[k] for k in utils.SITE_MODEL_COLUMNS}
    other.update(site=saved["site"], num_sites=n_sites)
    utils.save_site_model(f("other.npz"), other, ["transcript_A", "transcript_C"], [ln for _, ln in REFS])
    with pytest.raises(ValueError, match=r"--site-model .*other\.npz: the site model was fitted over other contigs than the BAM header's"):
        seg.main(base + ["-o", f("x.csv"), "--site-summary", f("x.tsv"), "--site-model", f("other.npz")])
    assert not os.path.exists(f("x.csv.zst")) and not os.path.exists(f("x.tsv"))
    # a sparse table too small for the model: the dropped model rows are reported (and, the table being full, the run's own rows
    # are dropped too: exit status 3, as --site-capacity has it)
    capfd.readouterr()
    with pytest.raises(SystemExit) as status:
        seg.main(base + ["-o", f("small.csv"), "--site-summary", f("small.tsv"), "--site-model", f("model.npz"), "--site-capacity", "8"])
    assert status.value.code == 3
    err = capfd.readouterr().err
    assert "site model: %s: %d positions loaded; %d of them found no row in the sparse table of 8 rows and were dropped" % (
        f("model.npz"), saved["site"].size, saved["site"].size - 8) in err
    assert rows_of(f("small.csv.zst"))[0] == h1


def test_refusals(models, tmp_path):
    pore = "rna002"
    model = model_for(models, pore)
    base = ["-r", str(tmp_path), "-b", str(tmp_path / "none.bam"), "--mode", "basic", "-p", pore, "--model_path", model, "-o", str(tmp_path / "x.csv")]
    with pytest.raises(ValueError, match=r"--site-model-out saves the fitted per-site mixtures: it needs --site-mixture"):
        seg.main(base + ["--site-model-out", str(tmp_path / "m.npz")])
    with pytest.raises(ValueError, match=r"--site-model scores every row against its position's model beside the per-site table: it needs --site-summary FILE"):
        seg.main(base + ["--site-model", str(tmp_path / "m.npz")])
    assert not (tmp_path / "x.csv.zst").exists()
