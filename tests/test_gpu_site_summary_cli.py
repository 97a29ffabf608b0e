"""GPU (-m gpu): dynamont-resquiggle --site-summary on a synthetic POD5 + MAPPED BAM of 40 reads over two contigs. The TSV must be
the bytes the restatement (tests/site_summary_cases.py) predicts from the CSV's OWN borders -- every row's start / end cut out of
the signal the pipeline aligned, keyed by the site of the row's base as the BAM's pos + CIGAR give it -- and the .csv must be
byte-equal to a run without the flag. No torch in this process (tests/conftest.py)."""
import os

import numpy as np
import pytest

import site_summary_cases as ssc
from conftest import model_for
from dynamont_amd import bam_io, synth, zstd_io
from dynamont_amd._dynamont import site_summary_from_limbs
from dynamont_amd.segmentation import segment as seg
from dynamont_amd.segmentation.utils import hampel, write_site_summary
from dynamont_amd.sites import DYN_SITE_NONE, cigar_words, contig_offsets, site_ids_from_cigar, to_aligner_orientation

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

REFS = [("transcript_A", 700), ("transcript_B", 450)]


def _mapping(i, l_seq, rng):
    """(flag, ref_id, pos, cigar words) of read i: mostly forward with clips, an insertion and a deletion; every eighth read one of
    reverse strand, unmapped, secondary, supplementary, the CG placeholder"""
    if i % 8 == 5:
        kind = (i // 8) % 5
        if kind == 1:
            return 4, -1, -1, []
        flag = (16, 4, 256, 2048, 0)[kind]
        cigar = "%dS%dN" % (l_seq, 40) if kind == 4 else "%dM" % l_seq
        return flag, i % 2, int(rng.integers(0, 100)), cigar_words(cigar).tolist()
    s0, s1, ins, dele = (int(v) for v in rng.integers(0, 6, 4))
    m = l_seq - s0 - s1 - ins
    a = int(rng.integers(5, m - 5))
    cigar = ("%dS" % s0 if s0 else "") + "%dM" % a + ("%dI" % ins if ins else "") + ("%dD" % dele if dele else "") + "%dM" % (m - a) + \
        ("%dS" % s1 if s1 else "")
    ref = i % 2
    return 0, ref, int(rng.integers(0, REFS[ref][1] - m - dele)), cigar_words(cigar).tolist()


def test_site_summary_tsv_equals_the_restatement_from_the_csvs_own_borders(models, tmp_path):
    pore = "rna002"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(6401, 40, pore, mean, sd, (60, 200))
    raw, bam, expected = synth.write_dataset(str(tmp_path / "in"), "ss", reads, pore, seed=6, container="pod5", basecalls="bam")
    recs = list(bam_io.iter_bam(bam))
    assert len(recs) == 40 == len(expected)
    rng = np.random.default_rng(64)
    maps = [_mapping(i, len(r.query_sequence), rng) for i, r in enumerate(recs)]
    mapped = str(tmp_path / "in" / "mapped.bam")
    bam_io.write_bam(mapped, [(r.query_name, r.query_sequence, r._tags, m) for r, m in zip(recs, maps)], references=REFS)
    base = ["-r", os.path.dirname(raw), "-b", mapped, "--mode", "basic", "-p", pore, "--model_path", model, "--batch-reads", "7"]
    tsv = str(tmp_path / "sites.tsv")
    seg.main(base + ["-o", str(tmp_path / "with.csv"), "--site-summary", tsv])
    seg.main(base + ["-o", str(tmp_path / "without.csv")])
    with_csv = open(str(tmp_path / "with.csv.zst"), "rb").read()
    assert with_csv == open(str(tmp_path / "without.csv.zst"), "rb").read()          # the flag changes no byte of the rows
    # the CSV's own borders, per read in the order of the BAM
    rows = {}
    lines = zstd_io.decompress(with_csv).decode().split("\n")
    assert lines[0].startswith("readid,signalid,start,end,basepos,") and lines[-1] == ""
    for ln in lines[1:-1]:
        p = ln.split(",")
        rows.setdefault(p[0], []).append((int(p[2]), int(p[3]), int(p[4])))
    assert len(rows) >= 36
    offs = contig_offsets([ln for _, ln in REFS])
    num_sites = int(offs[-1])
    acc = ssc.empty(num_sites)
    keyed = 0
    for rec, (flag, ref, pos, cigar), (x, seq) in zip(recs, maps, expected):
        if rec.query_name not in rows:
            continue
        x = x.copy()
        hampel(x)                                                    # the signal the pipeline aligned
        l_seq, L = len(rec.query_sequence), len(seq)
        placeholder = len(cigar) == 2 and cigar[1] & 0xF == 3
        if flag & (4 | 16 | 256 | 2048) or placeholder:
            ids = np.full(L, DYN_SITE_NONE, dtype=np.uint32)
        else:
            ids = to_aligner_orientation(site_ids_from_cigar(pos, cigar, l_seq, offs[ref]), True, L - l_seq)
            keyed += 1
        first = rec.get_tag("ts") + (rec.get_tag("sp") if rec.has_tag("sp") else 0)
        r = rows[rec.query_name]
        assert len(r) == L - 5 + 1 and r[-1][1] - first == len(x)
        ssc.add_read(acc, [int(ids[L - 1 - bp]) for _, _, bp in r], [x[a - first:b - first] for a, b, _ in r])
    assert keyed >= 30 and acc["totals"]["rows_without_site"] > 9 * keyed            # the pad's rows, the clips, the unkeyed reads
    assert (np.array(acc["n_rows"]) > 1).sum() > 200                                 # reads overlap on both contigs
    full = site_summary_from_limbs(*ssc.limbs(acc))
    want = str(tmp_path / "want.tsv")
    write_site_summary(want, lambda lo, hi: {k: (v[lo:hi] if k not in ("limbs", "totals") else v) for k, v in full.items()},
                       num_sites, [n for n, _ in REFS], offs)
    got = open(tsv).read()
    assert got == open(want).read()
    body = got.split("\n")[1:-1]
    assert len(body) == int((np.array(acc["n_rows"]) > 0).sum()) and {ln.split("\t")[0] for ln in body} == {n for n, _ in REFS}
    assert sum(int(ln.split("\t")[2]) for ln in body) == acc["totals"]["rows_added"]
    pos = [(ln.split("\t")[0], int(ln.split("\t")[1])) for ln in body]
    assert pos == sorted(pos) and min(p for _, p in pos) >= 1                         # reference order, 1-based
