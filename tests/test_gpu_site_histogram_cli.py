"""GPU (-m gpu): dynamont-resquiggle --site-summary F --site-histogram BINS[:LO:HI] on the synthetic POD5 + MAPPED BAM of
tests/test_gpu_site_summary_cli.py (40 reads over two contigs, built the same way). The three new columns must be the quantiles
restated (tests/site_histogram_cases.py) from the --event-stats rows of the same run, grouped by site on the host: every row's
event mean from its own borders (checked against the row's level_mean column), keyed by the site the BAM's pos + CIGAR give its
base. The first eight columns are those of a run without the flag; without LO:HI the range comes from the model table.
No torch in this process (tests/conftest.py)."""
import os
import re

import numpy as np
import pytest

import site_histogram_cases as shc
from conftest import model_for
from dynamont_amd import bam_io, synth, zstd_io
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel, site_histogram_range, site_quantile_levels
from dynamont_amd.sites import DYN_SITE_NONE, contig_offsets, site_ids_from_cigar, to_aligner_orientation
from test_gpu_site_summary_cli import REFS, _mapping

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


def site_means(csv_bytes, recs, maps, expected, offs):
    """{site: [event mean of every row keyed to it]} from the CSV's own rows"""
    rows = {}
    lines = zstd_io.decompress(csv_bytes).decode().split("\n")
    head = lines[0].split(",")
    assert head[:5] == ["readid", "signalid", "start", "end", "basepos"] and "level_mean" in head
    col = head.index("level_mean")
    for ln in lines[1:-1]:
        p = ln.split(",")
        rows.setdefault(p[0], []).append((int(p[2]), int(p[3]), int(p[4]), p[col]))
    out = {}
    for rec, (flag, ref, pos, cigar), (x, seq) in zip(recs, maps, expected):
        if rec.query_name not in rows:
            continue
        x = x.copy()
        hampel(x)                                                    # the signal the pipeline aligned
        l_seq, L = len(rec.query_sequence), len(seq)
        placeholder = len(cigar) == 2 and cigar[1] & 0xF == 3
        if flag & (4 | 16 | 256 | 2048) or placeholder:
            continue
        ids = to_aligner_orientation(site_ids_from_cigar(pos, cigar, l_seq, offs[ref]), True, L - l_seq)
        first = rec.get_tag("ts") + (rec.get_tag("sp") if rec.has_tag("sp") else 0)
        for a, b, bp, text in rows[rec.query_name]:
            sid = int(ids[L - 1 - bp])
            if sid == DYN_SITE_NONE:
                continue
            m = shc.row_mean(x[a - first:b - first])
            assert m is not None and "%.6f" % m == text              # the row's own level_mean column
            out.setdefault(sid, []).append(float(m))
    return out


def expected_columns(means, spec):
    """{site: the three column texts} by the definition: bin every mean, take the quantiles of the counts, interpolate on the host"""
    bins, lo, hi = spec
    out = {}
    for sid, ms in means.items():
        counts = [0] * (bins + 2)
        for m in ms:
            counts[shc.level_bin(m, bins, lo, hi)] += 1
        n, cols = shc.quantile_arrays([counts], (0.25, 0.5, 0.75))
        assert n[0] == len(ms)
        out[sid] = [repr(float(v)) for v in site_quantile_levels(cols[0], cols[1], cols[2], cols[3], bins, lo, hi)[0]]
    return out


def test_three_quantile_columns_equal_the_restatement_and_the_others_do_not_change(models, tmp_path, capfd):
    pore = "rna002"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(6401, 40, pore, mean, sd, (60, 200))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "sh", reads, pore, seed=6, container="pod5", basecalls="bam")
    recs = list(bam_io.iter_bam(bam))
    rng = np.random.default_rng(64)
    maps = [_mapping(i, len(r.query_sequence), rng) for i, r in enumerate(recs)]
    mapped = str(tmp_path / "in" / "mapped.bam")
    bam_io.write_bam(mapped, [(r.query_name, r.query_sequence, r._tags, m) for r, m in zip(recs, maps)], references=REFS)
    base = ["-r", os.path.dirname(raw), "-b", mapped, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "7", "--event-stats"]
    plain, fixed, auto = (str(tmp_path / f) for f in ("plain.tsv", "fixed.tsv", "auto.tsv"))
    seg.main(base + ["-o", str(tmp_path / "plain.csv"), "--site-summary", plain])
    seg.main(base + ["-o", str(tmp_path / "fixed.csv"), "--site-summary", fixed, "--site-histogram", "32:-4:4"])
    capfd.readouterr()
    seg.main(base + ["-o", str(tmp_path / "auto.csv"), "--site-summary", auto, "--site-histogram", "24"])
    err = capfd.readouterr().err
    csv = open(str(tmp_path / "fixed.csv.zst"), "rb").read()
    assert csv == open(str(tmp_path / "plain.csv.zst"), "rb").read() == open(str(tmp_path / "auto.csv.zst"), "rb").read()
    offs = contig_offsets([ln for _, ln in REFS])
    means = site_means(csv, recs, maps, expected, offs)
    assert len(means) > 400 and max(len(v) for v in means.values()) >= 5
    # without LO:HI the range is the model table's: four of its largest standard deviations beyond its extreme levels
    # (the handle's table in k-mer code order holds the file's values: min / max do not depend on the order)
    lo, hi = site_histogram_range(np.asarray(mean, dtype=np.float64), np.asarray(sd, dtype=np.float64))
    said = re.search(r"site histogram: 24 bins over \[(\S+), (\S+)\)", err)
    assert said and float(said.group(1)) == lo and float(said.group(2)) == hi and lo < -1.0 and hi > 1.0
    names = [n for n, _ in REFS]
    plain_lines = open(plain).read().split("\n")
    for path, spec in ((fixed, (32, -4.0, 4.0)), (auto, (24, lo, hi))):
        want = expected_columns(means, spec)
        got = open(path).read().split("\n")
        assert got[0] == plain_lines[0] + "\tlevel_q25\tlevel_median\tlevel_q75" and got[-1] == "" and len(got) == len(plain_lines)
        assert len(got) - 2 == len(want)
        seen_finite = 0
        for ln, pl in zip(got[1:-1], plain_lines[1:-1]):
            p = ln.split("\t")
            assert len(p) == 11 and p[:8] == pl.split("\t")            # the first eight columns: the run without the flag
            sid = int(offs[names.index(p[0])]) + int(p[1]) - 1
            assert p[8:] == want[sid], (path, p[0], p[1], p[8:], want[sid])
            assert int(p[2]) == len(means[sid])
            seen_finite += all(np.isfinite(float(v)) for v in p[8:])
        assert seen_finite > 0.9 * len(want)
