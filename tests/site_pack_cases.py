"""The per-site table by content (dyn_aligner_site_pack, dyn_aligner_site_summary_merge), restated with Python ints, and the
inputs of its device harness (tests/device_math/site_pack.hip).

The DEFINITION.
  pack    the table rows [row_lo, row_lo + count) in ascending order; the id of a row is the row itself (dense) or the bucket's key
          (sparse; 0xFFFFFFFF: an empty bucket has none). A row is LIVE iff it has an id, the id lies in [site_lo, site_hi) and any
          of its 7 cell words or of its counters is non-zero. The records: (id, the 7 words, the counters) of the live rows.
  merge   record (id, words, counters) adds into the row of id + offset: n_rows, n_samples, dwell_sq mod 2^64, M1 and M2 (words
          3, 4 and 5, 6 as low and high limb) mod 2^128, every counter mod 2^32. An all-zero record adds nothing and takes no row. A
          sparse table: a record whose id has no bucket (`present`) is dropped whole and counted.
"""
import numpy as np

EMPTY = 0xFFFFFFFF
M32, M64, M128 = (1 << 32) - 1, (1 << 64) - 1, (1 << 128) - 1
DWELL_BINS = 16
CHUNK_ROWS = 64          # asserted against the harness's sph_chunk_rows()
SCAN_TILE_ROWS = 65536   # asserted against the harness's sph_scan_tile_rows(): the rows one step of the scan covers


def width(bins):
    return bins + 2 + DWELL_BINS if bins else 0


def pack_reference(keys, cells, hist, row_lo, count, site_lo, site_hi):
    """keys: uint32 [rows] or None (dense); cells: uint64 [rows, 7]; hist: uint32 [rows, width] or None.
    Returns [(id, [7 ints], [width ints])] in ascending row order"""
    out = []
    rows = np.arange(row_lo, row_lo + count)
    # (the rows with a non-zero word, found at once: the loop below then states the rule on Python ints for those alone)
    some = np.asarray(cells)[rows].any(axis=1) | (np.asarray(hist)[rows].any(axis=1) if hist is not None else False)
    for row in rows[some].tolist():
        key = row if keys is None else int(keys[row])
        if key == EMPTY or not site_lo <= key < site_hi:
            continue
        words = cells[row].tolist()
        counters = hist[row].tolist() if hist is not None else []
        if any(words) or any(counters):
            out.append((key, words, counters))
    return out


def records_as_arrays(records, w):
    """the three arrays of the C interface: site uint32 [n], cells uint64 [n, 7], counters uint32 [n, w]"""
    n = len(records)
    site = np.array([r[0] for r in records], dtype=np.uint32).reshape(n)
    cells = np.array([r[1] for r in records], dtype=np.uint64).reshape(n, 7)
    counters = np.array([r[2] for r in records], dtype=np.uint32).reshape(n, w)
    return site, cells, counters


def merge_reference(table, records, offset=0, present=None):
    """adds the records into table = {id: ([7 words], [counters])} (in place); present: the keys a sparse map holds afterwards
    (None: every id has a row). Returns the number of records dropped"""
    dropped = 0
    for key, words, counters in records:
        if not any(words) and not any(counters):
            continue
        key += offset
        if present is not None and key not in present:
            dropped += 1
            continue
        w, c = table.setdefault(key, ([0] * 7, [0] * len(counters)))
        for f in range(3):
            w[f] = (w[f] + words[f]) & M64
        for lo in (3, 5):
            v = ((w[lo] | (w[lo + 1] << 64)) + (words[lo] | (words[lo + 1] << 64))) & M128
            w[lo], w[lo + 1] = v & M64, v >> 64
        for i, v in enumerate(counters):
            c[i] = (c[i] + v) & M32
    return dropped


# ---- tables of the harness -------------------------------------------------------------------------------------------------------
def random_rows(rng, rows, w, live):
    """cells uint64 [rows, 7] and hist uint32 [rows, w]: the rows of the boolean array `live` hold random words (every word of a
    live row non-zero), the others zeros"""
    cells = np.zeros((rows, 7), dtype=np.uint64)
    hist = np.zeros((rows, w), dtype=np.uint32)
    idx = np.flatnonzero(live)
    cells[idx] = rng.integers(1, 1 << 63, (idx.size, 7), dtype=np.uint64)
    if w:
        hist[idx] = rng.integers(1, 1 << 32, (idx.size, w), dtype=np.uint32)
    return cells, hist


LIVE_PATTERNS = ("none", "all", "alternating", "last")


def live_pattern(name, rows):
    live = np.zeros(rows, dtype=bool)
    if name == "all":
        live[:] = True
    elif name == "alternating":
        live[::2] = True
    elif name == "last" and rows:
        live[-1] = True
    return live
