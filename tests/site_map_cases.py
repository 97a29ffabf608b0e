"""The sparse mode of the per-site table (dyn_aligner_set_site_summary_sparse), restated with Python ints, and the inputs of its
device harness (tests/device_math/site_map.hip).

The DEFINITION. The table's cells are those of site_summary_cases, keyed by site id in a dict instead
of a list: the id space goes up to 4 294 967 294 whatever the memory. The MAP: uint32 keys[capacity], 0xFFFFFFFF empty, the bucket
is the row; the home bucket of an id comes from the harness's sm_home and from nothing else; linear probing with wrap-around over
at most min(capacity, 128) buckets. Nothing is ever deleted, so a key is in the map with ALL of its rows or absent with all of
them dropped -- which keys get in under overflow depends on the order of the atomics, what a present key's cell holds does not.

check_map() states what must hold of ANY map the device leaves, whatever that order:
  every key at most once; every key within its probe window of its home bucket with no empty bucket before it; an empty
  bucket's cell all zero; n_keys = the occupied buckets.
"""
import numpy as np

import site_histogram_cases as shc
import site_summary_cases as ssc

EMPTY = 0xFFFFFFFF
PROBE_MAX = 128          # asserted against the harness's smh_probe_max()
ID_SPACE = 4294967294    # the largest num_sites: ids 0 .. 4 294 967 293
FIELDS = ("n_rows", "n_samples", "dwell_sq", "M1", "M2")


# ---- the definition over a dict ---------------------------------------------------------------------------------------------
def empty():
    return {"cells": {}, "totals": dict.fromkeys(ssc.TOTALS, 0)}


def add_read(acc, ids, segments, num_sites=ID_SPACE, present=None, hist=None, spec=None):
    """one ok read. present: the keys the map holds (None: no row is dropped) -- a row of another key counts in rows_skipped and
    in the returned number of dropped rows. hist / spec: {id: (level list, dwell list)} and (bins, lo, hi)"""
    dropped = 0
    acc["totals"]["reads_ok"] += 1
    for s, x in zip(ids, segments):
        s = int(s)
        if s == EMPTY:
            acc["totals"]["rows_without_site"] += 1
            continue
        t = ssc.row_terms(x) if s < num_sites else None
        if t is not None and present is not None and s not in present:
            dropped += 1
            t = None
        if t is None:
            acc["totals"]["rows_skipped"] += 1
            continue
        L, m1, m2 = t
        c = acc["cells"].setdefault(s, [0, 0, 0, 0, 0])
        for f, v in enumerate((1, L, L * L, m1, m2)):
            c[f] += v
        acc["totals"]["rows_added"] += 1
        acc["totals"]["samples_added"] += L
        if hist is not None:
            bins, lo, hi = spec
            lv, dw = hist.setdefault(s, ([0] * (bins + 2), [0] * shc.DWELL_BINS))
            lv[shc.level_bin(shc.row_mean(x), bins, lo, hi)] += 1
            dw[shc.dwell_bin(len(x))] += 1
    return dropped


def reference(reads, num_sites=ID_SPACE, present=None, hist=None, spec=None, runs=1):
    """(table, dropped rows) of `runs` launches of the ok reads of [(status, [(id, samples)])]"""
    acc, dropped = empty(), 0
    for _ in range(runs):
        for status, segs in reads:
            if status == 0:
                dropped += add_read(acc, [s for s, _ in segs], [x for _, x in segs], num_sites, present, hist, spec)
    return acc, dropped


def cell_limbs(c):
    """the seven uint64 of one cell"""
    out = [c[0] & ssc.M64, c[1] & ssc.M64, c[2] & ssc.M64]
    for v in (c[3], c[4]):
        tw = v & ssc.M128
        out += [tw & ssc.M64, tw >> 64]
    return out


def from_limbs(w):
    """[n_rows, n_samples, dwell_sq, M1, M2] of seven uint64 as Python ints (M1, M2 signed)"""
    w = [int(v) for v in w]
    out = w[:3]
    for lo, hi in ((w[3], w[4]), (w[5], w[6])):
        v = lo | (hi << 64)
        out.append(v - (1 << 128) if v >> 127 else v)
    return out


# ---- what must hold of any map ------------------------------------------------------------------------------------------------
def check_map(keys, cells, n_keys, home, probe_max=PROBE_MAX):
    """keys uint32 [capacity], cells uint64 [capacity, 7], home(ids) -> home buckets. Returns {key: bucket}"""
    cap = len(keys)
    occ = np.flatnonzero(keys != EMPTY)
    assert n_keys == occ.size, (n_keys, occ.size)
    ks = keys[occ]
    assert np.unique(ks).size == ks.size, "a key sits in two buckets"
    assert not cells[keys == EMPTY].any(), "an empty bucket's cell is not zero"
    window = min(cap, probe_max)
    for b, k, h in zip(occ.tolist(), ks.tolist(), home(ks).tolist()):
        d = (b - h) % cap
        assert d < window, ("key outside its probe window", k, h, b)
        before = [(h + i) % cap for i in range(d)]
        assert (keys[before] != EMPTY).all(), ("an empty bucket before the key", k, h, b)
    return dict(zip(ks.tolist(), occ.tolist()))


# ---- batches --------------------------------------------------------------------------------------------------------------------
def scatter_ids(n=ssc.NUM_SITES, seed=20262):
    """site_summary_cases' ids 0 .. n - 1 sent injectively into the whole id space: id 0, the last id, ids at or above
    4 000 000 000, the rest anywhere; n itself (the batch's id outside the table) and NONE - 1 go to ID_SPACE, which is outside"""
    rng = np.random.default_rng(seed)
    ids = {0, ID_SPACE - 1, 4000000000, 4000000001}
    while len(ids) < n // 2:
        ids.add(int(rng.integers(4000000000, ID_SPACE)))
    while len(ids) < n:
        ids.add(int(rng.integers(0, ID_SPACE)))
    ids = np.array(sorted(ids), dtype=np.uint64)
    rng.shuffle(ids)
    table = {s: int(ids[s]) for s in range(n)}
    table[n] = ID_SPACE
    table[EMPTY - 1] = ID_SPACE
    table[EMPTY] = EMPTY
    return table


def remap(reads, table):
    return [(status, [(table[int(s)], x) for s, x in segs]) for status, segs in reads]


def same_home_ids(home, capacity, bucket, n, limit=1 << 22):
    """the first n ids below `limit` whose home bucket is `bucket`"""
    ids = np.arange(limit, dtype=np.uint32)
    hit = ids[home(ids, capacity) == bucket]
    assert hit.size >= n, (hit.size, n)
    return [int(v) for v in hit[:n]]


def contended_reads(keys, n_reads, per_wave, seed, long_rows=()):
    """n_reads reads whose row j belongs to key j // per_wave: `per_wave` consecutive rows (lanes of one wave) carry the same, new
    key, every key comes from every read (several blocks per read once len(keys) * per_wave > 256); rows of 1 .. 5 samples.
    long_rows: (key index, samples > 256) rows of one more read, for the block-per-read kernel"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_reads):
        reads.append((0, [(k, rng.normal(0.3, 1.0, int(rng.integers(1, 6)))) for k in keys for _ in range(per_wave)]))
    if long_rows:
        reads.append((0, [(keys[i], rng.normal(-0.2, 1.0, L)) for i, L in long_rows]))
    return reads


def pack(reads):
    return shc.pack(reads, num_sites=ID_SPACE)
