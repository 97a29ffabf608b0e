"""Site ids for the per-site level summary (``Aligner.set_site_summary``) from a read's mapping.

A site id is a uint32 per BASE of a read: usually the global index of the reference position the base is aligned to,
``contig_offsets(lengths)[ref_id] + position``. ``DYN_SITE_NONE`` marks a base without a site (an insertion, a soft clip, the
polyA pad the RNA pipeline adds). The ids reach the aligner in ALIGNER orientation, packed like the sequences:

    offs = contig_offsets(reference_lengths)
    ids = site_ids_from_cigar(pos, cigar, l_seq, offs[ref_id])          # stored (BAM) order, one per stored base
    ids = to_aligner_orientation(ids, aligner.rna, len(sequence) - l_seq)  # what the aligner's sequence looks like
    aligner.align_batch(signals, sequences, site_ids=np.concatenate(all_ids))

Everything here is plain numpy on the host; nothing touches the GPU.
"""
from __future__ import annotations

import numpy as np

DYN_SITE_NONE = 0xFFFFFFFF

# BAM's CIGAR operations, in the order of their codes: cigar word = length << 4 | code
CIGAR_OPS = "MIDNSHP=X"
_QUERY_AND_REF = (0, 7, 8)  # M = X: consecutive sites
_QUERY_ONLY = (1, 4)        # I S: bases without a site
_REF_ONLY = (2, 3)          # D N: the reference moves on
_NEITHER = (5, 6)           # H P


def cigar_words(ops) -> np.ndarray:
    """BAM's uint32 words from a CIGAR string ("5S20M1D3M"), a list of (op letter or code, length) pairs, or the words themselves"""
    if isinstance(ops, str):
        import re
        if ops in ("", "*"):
            return np.zeros(0, dtype=np.uint32)
        parts = re.findall(r"(\d+)([MIDNSHP=X])", ops)
        if "".join(n + c for n, c in parts) != ops:
            raise ValueError(f"not a CIGAR string: {ops!r}")
        return np.array([int(n) << 4 | CIGAR_OPS.index(c) for n, c in parts], dtype=np.uint32)
    if len(ops) and isinstance(ops[0], (tuple, list)):
        return np.array([int(n) << 4 | (CIGAR_OPS.index(c) if isinstance(c, str) else int(c)) for c, n in ops], dtype=np.uint32)
    return np.ascontiguousarray(ops, dtype=np.uint32)


def site_ids_from_cigar(pos: int, cigar_ops, l_seq: int, contig_offset: int = 0) -> np.ndarray:
    """uint32[l_seq], one id per base of the STORED sequence, in stored order. ``pos``: BAM's 0-based leftmost reference
    position; ``cigar_ops``: see ``cigar_words``; ``contig_offset``: what makes the position a global site index
    (``contig_offsets``). M, = and X take consecutive sites; I and S take ``DYN_SITE_NONE``; D and N advance the reference; H and
    P do nothing. ValueError when the CIGAR does not cover ``l_seq`` bases or a site does not fit below ``DYN_SITE_NONE``."""
    words = cigar_words(cigar_ops)
    ids = np.full(int(l_seq), DYN_SITE_NONE, dtype=np.uint32)
    q, ref = 0, int(contig_offset) + int(pos)
    for w in words.tolist():
        n, op = w >> 4, w & 0xF
        if op in _QUERY_AND_REF:
            if q + n <= l_seq:
                if ref < 0 or ref + n > DYN_SITE_NONE:
                    raise ValueError(f"site ids {ref} .. {ref + n - 1} do not fit a uint32 below DYN_SITE_NONE")
                ids[q:q + n] = np.arange(ref, ref + n, dtype=np.uint64).astype(np.uint32)
            q += n
            ref += n
        elif op in _QUERY_ONLY:
            q += n
        elif op in _REF_ONLY:
            ref += n
        elif op not in _NEITHER:
            raise ValueError(f"CIGAR operation code {op} is not one of BAM's nine")
    if q != l_seq:
        raise ValueError(f"the CIGAR covers {q} bases of the query, the stored sequence has {int(l_seq)}")
    return ids


def to_aligner_orientation(ids, rna: bool, pad_len_added: int = 0) -> np.ndarray:
    """The ids of a stored sequence as the aligner's sequence needs them: reversed for RNA (the pipeline aligns the reversed
    basecall), with ``pad_len_added`` x ``DYN_SITE_NONE`` in front for the polyA pad it prepended (0: the read had one)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    if pad_len_added < 0:
        raise ValueError("pad_len_added is negative")
    if rna:
        ids = ids[::-1]
    if pad_len_added:
        ids = np.concatenate([np.full(int(pad_len_added), DYN_SITE_NONE, dtype=np.uint32), ids])
    return np.ascontiguousarray(ids)


def contig_offsets(lengths) -> np.ndarray:
    """uint64[n + 1]: the prefix sums of the reference lengths. Site of (contig c, 0-based position p) = offsets[c] + p; the
    table needs ``num_sites = offsets[-1]`` entries."""
    out = np.zeros(len(lengths) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(lengths, dtype=np.uint64), out=out[1:])
    return out
