"""CPU: from a mapped BAM to site ids. dynamont_amd/sites.py against hand-worked CIGARs; the two BAM readers (the native one,
dyn_bam_references / dyn_bam_alignment, and bam_io's Python parser) on a mapped BAM the test assembles byte by byte: two
references, forward / reverse / unmapped / secondary records, one CIGAR across a BGZF block boundary; an unaligned BAM; a record
whose CIGAR does not fit it."""
import ctypes as C
import struct

import numpy as np
import pytest

from dynamont_amd import _native as N, bam_io
from dynamont_amd.sites import (CIGAR_OPS, DYN_SITE_NONE, cigar_words, contig_offsets, site_ids_from_cigar, to_aligner_orientation)

pytestmark = pytest.mark.usefixtures("native_lib")
X = DYN_SITE_NONE


# ---- sites.py ------------------------------------------------------------------------------------------------------------------
def test_every_op_by_hand():
    # 2S 3M 1I 2M 2D 1= 3N 1X 1H 1P at pos 10, contig offset 100: S S | 110 111 112 | I | 113 114 | (115 116 deleted) | 117 |
    # (118 119 120 skipped) | 121
    ids = site_ids_from_cigar(10, "2S3M1I2M2D1=3N1X1H1P", 10, 100)
    assert ids.dtype == np.uint32 and ids.tolist() == [X, X, 110, 111, 112, X, 113, 114, 117, 121]
    assert cigar_words("2S3M").tolist() == [2 << 4 | 4, 3 << 4 | 0] and CIGAR_OPS.index("=") == 7 and CIGAR_OPS.index("X") == 8
    assert site_ids_from_cigar(10, [("S", 2), ("M", 3)], 5, 100).tolist() == [X, X, 110, 111, 112]
    assert site_ids_from_cigar(10, np.array([2 << 4 | 4, 3 << 4 | 0], dtype=np.uint32), 5, 100).tolist() == [X, X, 110, 111, 112]


def test_leading_clip_trailing_insertion_and_a_skip():
    assert site_ids_from_cigar(0, "4S2M", 6).tolist() == [X, X, X, X, 0, 1]                  # a leading S does not move the reference
    assert site_ids_from_cigar(7, "3M2I", 5).tolist() == [7, 8, 9, X, X]                     # an I at the end
    assert site_ids_from_cigar(7, "2M1000N2M", 4).tolist() == [7, 8, 1009, 1010]             # an N (a spliced read)
    assert site_ids_from_cigar(5, "5H3M5H", 3).tolist() == [5, 6, 7]                         # hard clips hold no bases
    assert site_ids_from_cigar(0, "*", 0).tolist() == []


def test_what_does_not_fit_is_refused():
    with pytest.raises(ValueError, match="covers 4 bases"):
        site_ids_from_cigar(0, "4M", 5)
    with pytest.raises(ValueError, match="covers 6 bases"):
        site_ids_from_cigar(0, "4M2I", 5)
    with pytest.raises(ValueError, match="do not fit"):
        site_ids_from_cigar(0xFFFFFFFE, "2M", 2)
    assert site_ids_from_cigar(0xFFFFFFFD, "2M", 2).tolist() == [0xFFFFFFFD, 0xFFFFFFFE]       # the largest id is NONE - 1
    with pytest.raises(ValueError, match="not a CIGAR"):
        cigar_words("3M2")
    with pytest.raises(ValueError, match="not one of BAM's nine"):
        site_ids_from_cigar(0, np.array([1 << 4 | 9], dtype=np.uint32), 1)


def test_rna_orientation_with_and_without_an_added_pad():
    stored = site_ids_from_cigar(20, "1S4M", 5)
    assert stored.tolist() == [X, 20, 21, 22, 23]
    assert to_aligner_orientation(stored, False).tolist() == [X, 20, 21, 22, 23]             # DNA: as stored
    assert to_aligner_orientation(stored, True).tolist() == [23, 22, 21, 20, X]              # RNA: reversed, the read had its pad
    assert to_aligner_orientation(stored, True, 3).tolist() == [X, X, X, 23, 22, 21, 20, X]  # ... or got 3 bases of pad in front
    assert to_aligner_orientation(stored, False, 2).tolist() == [X, X, X, 20, 21, 22, 23]
    out = to_aligner_orientation(stored, True, 9)
    assert out.dtype == np.uint32 and out.flags.c_contiguous and len(out) == 14
    with pytest.raises(ValueError, match="negative"):
        to_aligner_orientation(stored, True, -1)


def test_two_contigs():
    offs = contig_offsets([1000, 500])
    assert offs.dtype == np.uint64 and offs.tolist() == [0, 1000, 1500]
    assert site_ids_from_cigar(998, "2M", 2, offs[0]).tolist() == [998, 999]
    assert site_ids_from_cigar(0, "2M", 2, offs[1]).tolist() == [1000, 1001]                  # contig 1 starts where contig 0 ends
    assert site_ids_from_cigar(498, "2M", 2, int(offs[1])).max() == offs[-1] - 1              # num_sites = offs[-1]
    assert contig_offsets([]).tolist() == [0]


# ---- the readers ---------------------------------------------------------------------------------------------------------------
REFS = [("chrA", 1000), ("transcript_B", 500)]
TAGS = dict(qs=12.5, ns=5000, ts=10, fn="reads.pod5", sm=90.0, sd=15.0)


def _record(name, seq, flag, ref, pos, cigar, n_cigar=None):
    nm = name.encode() + b"\0"
    lut = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
    codes = [lut[c] for c in seq] + [0] * (len(seq) % 2)
    packed = bytes((codes[i] << 4) | codes[i + 1] for i in range(0, len(codes), 2))
    words = cigar_words(cigar)
    tagb = b""
    for k, v in TAGS.items():
        tagb += k.encode() + (b"f" + struct.pack("<f", v) if isinstance(v, float) else b"i" + struct.pack("<i", v) if isinstance(v, int)
                              else b"Z" + v.encode() + b"\0")
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(nm), 60, 4680, len(words) if n_cigar is None else n_cigar, flag, len(seq), -1, -1, 0)
    body += nm + words.astype("<u4").tobytes() + packed + b"\xff" * len(seq) + tagb
    return struct.pack("<i", len(body)) + body


RECORDS = [  # name, sequence, flag, ref_id, pos, CIGAR
    ("fwd", "ACGTACGTAC", 0, 0, 100, "2S6M1I1M"),
    ("rev", "TTGCATTGCA", 16, 1, 7, "4M2D6M"),
    ("unmapped", "ACGTAC", 4, -1, -1, "*"),
    ("secondary", "ACGTACGT", 256, 0, 300, "8M"),
    ("across", "GGGTTTAAACCC", 0, 1, 40, "1S2M1I2M1D2M1N2M1X1="),
]


def _write(path, refs, records, split_in_cigar_of=None):
    head = b"BAM\x01"
    text = b"@HD\tVN:1.6\tSO:unknown\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n.encode(), ln) for n, ln in refs)
    head += struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for n, ln in refs:
        head += struct.pack("<i", len(n) + 1) + n.encode() + b"\0" + struct.pack("<i", ln)
    stream, cut = head, None
    for i, rec in enumerate(records):
        if i == split_in_cigar_of:
            cut = len(stream) + 4 + 32 + len(RECORDS[i][0]) + 1 + 4 * 3 + 2        # inside the fourth CIGAR word of that record
        stream += rec
    parts = [stream] if cut is None else [stream[:cut], stream[cut:]]
    with open(path, "wb") as w:
        for p in parts:
            w.write(bam_io._bgzf_block(p))
        w.write(bam_io._bgzf_block(b""))


@pytest.fixture(scope="module")
def mapped(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bam") / "mapped.bam")
    _write(path, REFS, [_record(*r) for r in RECORDS], split_in_cigar_of=4)
    blocks = open(path, "rb").read().count(b"\x1f\x8b\x08\x04")
    assert blocks == 3                                                # two data blocks (the cut) and the EOF marker
    return path


def test_both_readers_read_the_mapping(mapped):
    recs = list(bam_io.iter_bam(mapped))
    assert [r.query_name for r in recs] == [r[0] for r in RECORDS] and [r.query_sequence for r in recs] == [r[1] for r in RECORDS]
    rd = bam_io.NativeBamJobs(mapped)
    names, lengths = rd.references()
    assert names == [n for n, _ in REFS] and lengths.tolist() == [ln for _, ln in REFS] and lengths.dtype == np.uint32
    assert bam_io.bam_references(mapped) == (names, lengths.tolist())
    jb = rd.next(100)
    assert jb.n == len(RECORDS) and [jb.name(i) for i in range(jb.n)] == [r[0] for r in RECORDS]
    al = rd.alignment()
    assert al["cigar_off"].dtype == np.uint64 and len(al["cigar_off"]) == jb.n + 1 and al["cigar_off"][0] == 0
    for i, (name, seq, flag, ref, pos, cigar) in enumerate(RECORDS):
        words = cigar_words(cigar).tolist()
        a, b = int(al["cigar_off"][i]), int(al["cigar_off"][i + 1])
        assert (int(al["flag"][i]), int(al["ref_id"][i]), int(al["pos"][i]), al["cigar"][a:b].tolist()) == (flag, ref, pos, words), name
        assert (recs[i].flag, recs[i].ref, recs[i].pos, recs[i].cigar.tolist()) == (flag, ref, pos, words), name   # the Python parser
        assert recs[i].get_tag("ns") == 5000 and jb.bases[i] == len(seq)
    # from there to site ids: the forward read on contig 0, the read on contig 1 behind contig 0's 1000 sites
    offs = contig_offsets(lengths)
    a, b = int(al["cigar_off"][0]), int(al["cigar_off"][1])
    assert site_ids_from_cigar(al["pos"][0], al["cigar"][a:b], jb.bases[0], offs[al["ref_id"][0]]).tolist() == \
        [X, X, 100, 101, 102, 103, 104, 105, X, 106]
    a, b = int(al["cigar_off"][4]), int(al["cigar_off"][5])
    assert site_ids_from_cigar(al["pos"][4], al["cigar"][a:b], jb.bases[4], offs[al["ref_id"][4]]).tolist() == \
        [X, 1040, 1041, X, 1042, 1043, 1045, 1046, 1048, 1049, 1050, 1051]
    # a batch at a time: the columns are those of the LAST batch
    rd2 = bam_io.NativeBamJobs(mapped)
    assert rd2.alignment()["flag"].size == 0 and rd2.alignment()["cigar_off"].tolist() == [0]
    rd2.next(2)
    rd2.next(2)
    al2 = rd2.alignment()
    assert al2["flag"].tolist() == [4, 256] and al2["pos"].tolist() == [-1, 300] and al2["cigar"].tolist() == [8 << 4]
    assert al2["cigar_off"].tolist() == [0, 0, 1]
    rd.close()
    rd2.close()


def test_rna_orientation_keeps_the_mapping_in_bam_order(mapped):
    rd = bam_io.NativeBamJobs(mapped, rna=True, pad="AAAAAAAAA")
    jb = rd.next(100)
    al = rd.alignment()
    assert jb.read(0) == "AAAAAAAAA" + RECORDS[0][1][::-1] and al["cigar"][:4].tolist() == cigar_words(RECORDS[0][5]).tolist()
    stored = site_ids_from_cigar(al["pos"][0], al["cigar"][:4], jb.bases[0])
    ids = to_aligner_orientation(stored, True, len(jb.read(0)) - int(jb.bases[0]))
    assert len(ids) == len(jb.read(0)) and ids[:9].tolist() == [X] * 9 and ids[9:].tolist() == stored[::-1].tolist()
    rd.close()


def test_unaligned_bam_has_no_references_and_empty_cigars(tmp_path):
    path = str(tmp_path / "u.bam")
    bam_io.write_bam(path, [("r%d" % i, "ACGTACGT", dict(TAGS)) for i in range(3)])
    rd = bam_io.NativeBamJobs(path)
    names, lengths = rd.references()
    assert names == [] and lengths.size == 0 and bam_io.bam_references(path) == ([], [])
    assert rd.next(10).n == 3
    al = rd.alignment()
    assert al["flag"].tolist() == [4, 4, 4] and al["ref_id"].tolist() == [-1] * 3 and al["pos"].tolist() == [-1] * 3
    assert al["cigar"].size == 0 and al["cigar_off"].tolist() == [0, 0, 0, 0]
    assert all(r.cigar.size == 0 and r.flag == 4 and r.ref == -1 for r in bam_io.iter_bam(path))
    rd.close()


def test_a_cigar_that_does_not_fit_its_record_is_refused(tmp_path, native_lib):
    """n_cigar says 2 000 words, the record holds three: DYN_ERR_RUNTIME from the record check, before any word is read"""
    path = str(tmp_path / "bad.bam")
    _write(path, REFS, [_record(*RECORDS[0]), _record("short", "ACGT", 0, 0, 5, "1M1I2M", n_cigar=2000)])
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    assert native_lib.dyn_bam_open(path.encode(), 2, b"", C.byref(h), err, 512) == N.DYN_OK
    b = N.DynJobBatch()
    assert native_lib.dyn_bam_next(h, 10, 0, 0.0, 0, 1, C.byref(b), err, 512) == N.DYN_ERR_RUNTIME
    assert b"malformed BAM record" in err.value
    native_lib.dyn_bam_close(h)
    with pytest.raises(ValueError, match="malformed BAM record"):
        list(bam_io.iter_bam(path))
    assert native_lib.dyn_bam_alignment(None, None) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_bam_references(None, None, None, None, None) == N.DYN_ERR_INVALID_ARGUMENT
