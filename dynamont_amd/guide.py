"""Guide paths for the guided band (``Aligner.align_batch_guided`` / ``Batch.set_guide``). Pure NumPy,
no GPU, no library.

A guide is an int32 array with one entry per signal sample of a read: entry ``s`` is the lattice column (0 .. N-1, N = k-mers
+ 1) the window of lattice row ``s + 1`` is centred on. It never decreases. Lattice column ``j + 1`` is k-mer ``j`` of the
aligner's sequence (output row ``j``); column 0 is the lattice's start and holds only row 0.
"""
from __future__ import annotations

import numpy as np


def diagonal_guide(n_samples: int, n_columns: int) -> np.ndarray:
    """The reference's own band centre ``size_t(t * (N / T))`` for the lattice rows t = 1 .. n_samples (T = n_samples + 1,
    N = n_columns): one fp64 quotient, one fp64 product per row, truncated -- the same operations in the same order. A batch
    guided by it at ``half_width = min(band // 2, N // 2)`` is the unguided batch, bit for bit."""
    S, N = int(n_samples), int(n_columns)
    ratio = float(N) / float(S + 1)
    return (np.arange(1, S + 1, dtype=np.float64) * ratio).astype(np.int32)


def guide_from_starts(starts, n_samples: int, n_columns: int) -> np.ndarray:
    """``starts[j]``: the sample at which lattice column ``j + 1`` (k-mer ``j``) is expected to begin, non-decreasing. The
    centre of sample ``s`` is the number of starts ``<= s`` -- the column expected to be open at that sample -- clamped to
    ``[0, n_columns - 1]``. Starts past the last sample never count; more starts than columns pile up on the last column."""
    st = np.asarray(starts, dtype=np.int64).ravel()
    if st.size > 1 and (np.diff(st) < 0).any():
        raise ValueError("guide_from_starts: starts must be non-decreasing")
    S, N = int(n_samples), int(n_columns)
    if N < 1:
        raise ValueError("guide_from_starts: n_columns >= 1 is required")
    c = np.searchsorted(st, np.arange(S, dtype=np.int64), side="right")
    return np.clip(c, 0, N - 1).astype(np.int32)


def base_starts_from_moves(mv, ts: int = 0) -> np.ndarray:
    """Sample at which each base of a dorado move table (``mv:B:c``) starts: ``mv[0]`` is the stride, ``mv[1:]`` one flag per
    stride block, and base ``b`` starts at ``ts + stride * (index of the b-th set flag)``."""
    mv = np.asarray(mv).ravel()
    if mv.size < 1 or int(mv[0]) < 1:
        raise ValueError("guide_from_moves: mv[0] must be the stride (>= 1)")
    return int(ts) + int(mv[0]) * np.flatnonzero(mv[1:] != 0).astype(np.int64)


def guide_from_moves(mv, n_samples: int, n_bases: int, k: int, ts: int = 0, reverse: bool = False) -> np.ndarray:
    """Guide of a read from its basecaller move table.

    ``mv``: the ``mv:B:c`` tag as ``bam_io`` decodes it (``mv[0]`` the stride, ``mv[1:]`` the flags); base ``b`` in MOVE ORDER
    (= signal order) starts at ``ts + stride * (index of the b-th set flag)``, in samples of the signal the aligner is given
    (``ts``: where the move table's first block lies in that signal; 0 when the signal was cut at the basecaller's trim
    point). ``n_bases``: length of the aligner's sequence; k-mer ``j`` (lattice column ``j + 1``) takes the start of base
    ``j + k // 2``, its centre base. ``n_samples``: length of the aligner's signal.

    Orientation. The move table counts bases in signal order. ``reverse=False``: base ``b`` of the
    aligner's sequence is the ``b``-th base in signal order -- DNA basecalls as written, and RNA basecalls AFTER the front end
    has reversed them into the aligner's 3'->5' orientation. ``reverse=True``: the aligner's sequence runs against the move
    table's order and its signal is the time-reversed one: base ``b`` is move ``n - 1 - b`` and begins, in reversed samples,
    where that move ended (``n_samples -`` the next move's start).

    A sequence with more bases than the table has moves (the polyA pad the RNA front end prepends) gives the leading extra
    bases the first move's start; moves beyond the sequence are ignored."""
    S, L, k = int(n_samples), int(n_bases), int(k)
    n_kmers = L - k + 1
    if n_kmers < 1:
        raise ValueError("guide_from_moves: n_bases >= k is required")
    st = base_starts_from_moves(mv, ts)
    if st.size == 0:
        raise ValueError("guide_from_moves: the move table holds no move")
    if reverse:
        ends = np.append(st[1:], S)                      # move b ends where move b + 1 starts
        st = np.maximum(S - ends[::-1], 0)               # reversed samples, first base of the reversed order first
    if st.size < L:
        st = np.concatenate([np.full(L - st.size, st[0], dtype=np.int64), st])
    base_of_kmer = np.arange(n_kmers) + k // 2
    return guide_from_starts(st[base_of_kmer], S, n_kmers + 1)
