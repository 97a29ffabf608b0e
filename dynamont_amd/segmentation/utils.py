"""Counterpart of the reference's ``src/dynamont/segmentation/utils.py`` (names, arguments and
outputs kept; plotting helpers are out of scope).

Parity pins: tests/test_harness.py against tests/golden/g6_harness.npz (bytes produced by the
reference's own functions) and the reference tests' known-answer vectors
(tests/test_segment.py:179-200, tests/test_utils.py:7-114 of the reference).
"""
from __future__ import annotations

import sys
from os.path import dirname, join

import numpy as np

from dynamont_amd import Aligner

MAD_TO_SIGMA = 1.4826


def hampel(signal: np.ndarray, WINDOW: int = 3, n_sigmas: float = 3.0) -> None:
    """In-place Hampel filter with the reference's exact footprint (utils.py:16-43):
    windows are taken from the UNFILTERED signal; centre i = WINDOW//2 + w for window w;
    ``len - WINDOW - (WINDOW even)`` windows are examined, so the first WINDOW//2 and the last
    WINDOW//2 + 1 samples are never touched; a centre is replaced by its window median when
    |x - median| > n_sigmas * 1.4826 * MAD. No-op when size <= WINDOW."""
    size = signal.size
    if size <= WINDOW:
        return
    n_windows = size - WINDOW - (1 if WINDOW % 2 == 0 else 0)
    if n_windows <= 0:
        return
    src = signal.copy()
    half = WINDOW // 2
    win = np.lib.stride_tricks.sliding_window_view(src, WINDOW)[:n_windows]

    def row_median(a):
        s = np.sort(a, axis=1)
        if WINDOW % 2:
            return s[:, half].copy()
        return (s[:, half - 1] + s[:, half]) / 2.0

    med = row_median(win)
    mad = row_median(np.abs(win - med[:, None]))
    centre = src[half:half + n_windows]
    outlier = np.abs(centre - med) > n_sigmas * (MAD_TO_SIGMA * mad)
    view = signal[half:half + n_windows]
    view[outlier] = med[outlier]


def cnt_nts(sequence):
    """utils.py:45-61"""
    return {b: sequence.count(b) for b in "ACGT"}


def cnt_nts_ratios(sequence):
    """utils.py:63-79"""
    n = len(sequence)
    return {b: sequence.count(b) / n for b in "ACGT"}


class SegmentationError(Exception):
    """Raised when no segmentation was calculated for a read (utils.py:81-86)."""

    def __init__(self, read) -> None:
        self.read = read
        self.message = f"No segmentation calculated for {read}"
        super().__init__(self.message)


def get_model(pore: str) -> str:
    """Default model path per pore (utils.py:96-117); unknown keys are returned as a path."""
    models = {
        "rna002": "models/rna/rna002/rna002_5mer.model",
        "rna004": "models/rna/rna004/rna004_9mer.model",
        "dna_r10_260bps": "models/dna/r10.4.1/dna_r10.4.1_e8.2_260bps.model",
        "dna_r10_400bps": "models/dna/r10.4.1/dna_r10.4.1_e8.2_400bps.model",
    }
    base_dir = dirname(dirname(dirname(__file__)))
    return join(base_dir, models.get(pore, pore))


def read_kmer_model(file: str) -> dict:
    """{kmer: (mean, stdev)} from the TSV columns ``kmer, level_mean, level_stdv`` (utils.py:119-134)."""
    out = {}
    with open(file) as f:
        header = f.readline().rstrip("\n").split("\t")
        ik, im, isd = header.index("kmer"), header.index("level_mean"), header.index("level_stdv")
        for line in f:
            if not line.strip():
                continue
            p = line.rstrip("\n").split("\t")
            out[p[ik]] = (float(p[im]), float(p[isd]))
    return out


def write_kmer_model(file: str, kmer_model: dict) -> None:
    """utils.py:136-152: header + f'{kmer}\\t{mean}\\t{stdev}\\n' rows (repr-style floats)."""
    with open(file, "w") as w:
        w.write("kmer\tlevel_mean\tlevel_stdv\n")
        for kmer, (mean, stdev) in ((k, (v[0], v[1])) for k, v in kmer_model.items()):
            w.write(f"{kmer}\t{mean}\t{stdev}\n")


def write_kmer_model_arrays(file: str, kmers: bytes, k: int, mean, stdev) -> None:
    """write_kmer_model for values that already are arrays in file order (``kmers``: the rows' k-mer strings back to
    back): the same bytes, formatted by the library (dyn_format_model) -- 262 144 rows take 25 ms instead of 0.25 s."""
    import ctypes as C
    from .. import _native as N
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    stdev = np.ascontiguousarray(stdev, dtype=np.float64)
    n = len(mean)
    assert len(stdev) == n and len(kmers) == n * k
    L = N.lib()
    cap = int(L.dyn_format_model(kmers, k, mean.ctypes.data_as(N.c_double_p), stdev.ctypes.data_as(N.c_double_p), n, None, 0))
    buf = C.create_string_buffer(cap)
    used = int(L.dyn_format_model(kmers, k, mean.ctypes.data_as(N.c_double_p), stdev.ctypes.data_as(N.c_double_p), n, buf, cap))
    with open(file, "wb") as w:
        w.write(memoryview(buf)[:used])


def _make_native_aligner(model: str, params: dict, mode: str, device=None) -> Aligner:
    """utils.py:154-161"""
    pore = params.get("r") or params.get("pore")
    if pore is None:
        raise ValueError("Missing pore type in segmentation parameters")
    return Aligner(model, pore, mode=mode, threads=int(params.get("t", 1)), band=int(params.get("band", 400)),
                   device=device)


def _state_char(state) -> str:
    if isinstance(state, bytes):
        return state.decode("ascii")
    if isinstance(state, str):
        return state
    if isinstance(state, (int, np.integer)):
        return chr(int(state))
    return str(state)


def segmentation_to_string(result: dict, readid: str, signalid: str, sigOffset: int, lastIndex: int,
                           read: str, kmerSize: int, rna: bool, levels=None) -> bytes:
    """CSV rows of one read (utils.py:193-232): ``readid,signalid,start,end,basepos,base,motif,
    state,posterior_probability,polish``. ``read`` is in aligner orientation; for RNA the motif is
    reversed and basepos flipped AFTER ``base`` was taken. ``levels`` = (level_mean, level_stdv, level_median) of
    the read's segments (Aligner.set_event_stats): every row gets ``,{mean:.6f},{stdv:.6f},{median:.6f}`` after
    ``polish`` -- the rows dyn_format_csv_events writes."""
    seq_pos = result["sequence_positions"]
    sig_pos = result["signal_positions"]
    probs = result["probabilities"]
    states = result["states"]
    polishes = result.get("polishes")
    n = len(seq_pos)
    half = kmerSize // 2
    L = len(read)
    rows = []
    for i in range(n):
        bp = int(seq_pos[i])
        start = int(sig_pos[i]) + sigOffset
        end = int(sig_pos[i + 1]) + sigOffset if i + 1 < n else lastIndex
        motif = read[max(0, bp - half):min(L, bp + half + 1)]
        base = read[bp]
        polish = str(polishes[i]) if polishes is not None and polishes[i] else "NA"
        if rna:
            motif = motif[::-1]
            bp = L - bp - 1
        ev = "" if levels is None else f",{float(levels[0][i]):.6f},{float(levels[1][i]):.6f},{float(levels[2][i]):.6f}"
        rows.append(f"{readid},{signalid},{start},{end},{bp},{base},{motif},{_state_char(states[i])},"
                    f"{float(probs[i]):.6f},{polish}{ev}\n")
    return "".join(rows).encode("utf-8")


def train_transition_emission(signal, read, params, script, model, signalid, aligner: Aligner | None = None):
    """Single-read form of utils.py:163-182, kept for API parity. The k-mer <-> parameter pairing
    is by k-mer CODE (``Aligner.kmer_of_code``); the reference zips file order with code order,
    which mislabels RNA models."""
    try:
        al = aligner or _make_native_aligner(model, params, script)
        if script == "basic":
            res = al.train_batch([signal], [read])
            if res.status[0]:
                raise RuntimeError(res.error(0))
            t = res.transitions[:3]
            code, mean, sd = res.sparse(0)
            new_models = dict(read_kmer_model(model))
            for c, m, s in zip(code, mean, sd):
                new_models[kmer_of_code(int(c), al.kmer_size, al.rna)] = (float(m), float(s))
            return {"m1": float(t[0]), "e1": float(t[1]), "e2": float(t[2])}, new_models, float(res.Z[0])
        result = al.align(signal, read, calc_probabilities=False)
        trans = {k: float(v) for k, v in params.items() if k not in {"r", "t", "band"}}
        return trans, read_kmer_model(model), float(result["Z"])
    except Exception as error:
        print(f"error: native, {error} T: {len(signal)} N: {len(read)} Sid: {signalid}", file=sys.stderr)
        return signalid


def calcZ(signal, read, params, script, model, signalid, aligner: Aligner | None = None):
    """utils.py:184-191"""
    try:
        al = aligner or _make_native_aligner(model, params, script)
        return float(al.align(signal, read, calc_probabilities=False)["Z"])
    except Exception as error:
        print(f"error: native, {error} T: {len(signal)} N: {len(read)} Sid: {signalid}", file=sys.stderr)
        return signalid


def kmer_of_code(code: int, k: int, rna: bool) -> str:
    """intToKmer (aligner.cpp:222-239): base-4 digits, reversed back to 5'->3' for RNA."""
    s = []
    for _ in range(k):
        s.append("ACGT"[code % 4])
        code //= 4
    kmer = "".join(reversed(s))
    return kmer[::-1] if rna else kmer


def code_of_kmer(kmer: str, rna: bool) -> int:
    """inverse of kmer_of_code"""
    code = 0
    for ch in (kmer[::-1] if rna else kmer):
        code = code * 4 + "ACGT".index(ch)
    return code


def merge_kmer_summaries(parts: list) -> dict:
    """The sum of several Aligner.kmer_summary() results (the ranks of a multi-GPU run), added as Python ints: integer
    addition commutes, so the sum does not depend on how the reads were dealt out."""
    from dynamont_amd._dynamont import KMER_SUMMARY_TOTALS
    n = len(parts[0]["n_segments"])
    out = {"n_segments": np.zeros(n, dtype=np.uint64), "n_samples": np.zeros(n, dtype=np.uint64),
           "Q1": np.array([0] * n, dtype=object), "Q2": np.array([0] * n, dtype=object),
           "totals": dict.fromkeys(KMER_SUMMARY_TOTALS, 0)}
    for p in parts:
        out["n_segments"] = out["n_segments"] + p["n_segments"]
        out["n_samples"] = out["n_samples"] + p["n_samples"]
        out["Q1"] = out["Q1"] + p["Q1"]
        out["Q2"] = out["Q2"] + p["Q2"]
        for k in KMER_SUMMARY_TOTALS:
            out["totals"][k] += p["totals"][k]
    return out


def kmer_summary_table(summary: dict, model_mean, model_stdev) -> dict:
    """The derived columns of a per-k-mer summary (Aligner.kmer_summary), in k-mer-code order, each formed from the exact
    integers with one fp64 operation per step:
        m1 = float(Q1) * 2**-40 (int -> float correctly rounded), level_mean = m1 / n_samples,
        ex2 = float(Q2) * 2**-40 / n_samples, level_stdv = sqrt(max(0.0, ex2 - level_mean * level_mean)),
        dwell_mean = n_samples / n_segments.
    A k-mer the run never met (n_segments == 0) or met with zero variance carries the MODEL's mean and stdev in
    ``level_mean`` / ``level_stdv`` (``fitted`` is False there), so the table is always a loadable model."""
    import math
    n = len(summary["n_segments"])
    mm = np.asarray(model_mean, dtype=np.float64)
    ms = np.asarray(model_stdev, dtype=np.float64)
    assert len(mm) == n and len(ms) == n
    mean, stdv, dwell = mm.copy(), ms.copy(), np.zeros(n)
    fitted = np.zeros(n, dtype=bool)
    nseg, nsamp = summary["n_segments"].tolist(), summary["n_samples"].tolist()
    scale = 2.0 ** -40
    for c in np.flatnonzero(summary["n_segments"]).tolist():
        ns = float(nsamp[c])
        lm = float(summary["Q1"][c]) * scale / ns
        ex2 = float(summary["Q2"][c]) * scale / ns
        sd = math.sqrt(max(0.0, ex2 - lm * lm))
        dwell[c] = ns / float(nseg[c])
        if sd > 0.0:
            mean[c], stdv[c], fitted[c] = lm, sd, True
    return {"level_mean": mean, "level_stdv": stdv, "n_segments": summary["n_segments"], "n_samples": summary["n_samples"],
            "dwell_mean": dwell, "model_mean": mm, "model_stdv": ms, "fitted": fitted}


KMER_SUMMARY_HEADER = "kmer\tlevel_mean\tlevel_stdv\tn_segments\tn_samples\tdwell_mean\tmodel_mean\tmodel_stdv\n"


def write_kmer_summary(path: str, summary: dict, model_file: str, model_mean, model_stdev, rna: bool) -> dict:
    """The per-k-mer summary as a TSV in ``model_file``'s own k-mer order and orientation (floats as ``repr``). Its first
    three columns are a model file: ``read_kmer_model(path)`` and ``Aligner(path, pore)`` load it -- a hard-EM (Viterbi
    path) re-estimate of the model, with the model's own values where the run has none. ``model_mean`` / ``model_stdev``:
    the table the run aligned with, in k-mer-code order (Aligner.model_table()). Returns the table written."""
    t = kmer_summary_table(summary, model_mean, model_stdev)
    with open(model_file) as f:
        header = f.readline().rstrip("\n").split("\t")
        ik = header.index("kmer")
        names = [line.split("\t")[ik].strip() for line in f if line.strip()]
    nseg, nsamp = t["n_segments"].tolist(), t["n_samples"].tolist()
    cols = [t[k].tolist() for k in ("level_mean", "level_stdv", "dwell_mean", "model_mean", "model_stdv")]
    with open(path, "w") as w:
        w.write(KMER_SUMMARY_HEADER)
        for name in names:
            c = code_of_kmer(name, rna)
            w.write(f"{name}\t{cols[0][c]!r}\t{cols[1][c]!r}\t{nseg[c]}\t{nsamp[c]}\t{cols[2][c]!r}\t{cols[3][c]!r}\t{cols[4][c]!r}\n")
    return t


# ---- per-site level summary (Aligner.set_site_summary, dynamont-resquiggle --site-summary) -------------------------------------
SITE_SUMMARY_HEADER = "contig\tposition\tcoverage\tn_samples\tdwell_mean\tdwell_sd\tlevel_mean\tlevel_sd\n"


def site_summary_row(n_rows: int, n_samples: int, dwell_sq: int, M1: int, M2: int):
    """(dwell_mean, dwell_sd, level_mean, level_sd) of one site with coverage ``n_rows`` > 0, from the table's Python ints
    (INTEGRATION.md section 3). Every quantity is formed exactly, as a fraction, and rounded to a double once; the two standard
    deviations are the square roots of those doubles: level_mean = M1 / (n 2^40), level variance = M2 / (n 2^40) - (M1 / (n 2^40))^2,
    dwell_mean = n_samples / n, dwell variance = dwell_sq / n - (n_samples / n)^2, negative variances taken as 0."""
    from fractions import Fraction
    import math
    n = int(n_rows)
    lm = Fraction(int(M1), n << 40)
    lv = max(Fraction(0), Fraction(int(M2), n << 40) - lm * lm)
    dm = Fraction(int(n_samples), n)
    dv = max(Fraction(0), Fraction(int(dwell_sq), n) - dm * dm)
    return float(dm), math.sqrt(float(dv)), float(lm), math.sqrt(float(lv))


def site_summary_lines(summary: dict, lo: int, ref_names, offsets) -> list:
    """the TSV lines (no header) of the sites with coverage > 0 of one window ``summary`` = Aligner.site_summary(lo, hi), in
    reference order; ``offsets`` = sites.contig_offsets(reference lengths), positions 1-based"""
    out = []
    offs = np.asarray(offsets, dtype=np.int64)
    for i in np.flatnonzero(summary["n_rows"]).tolist():
        site = lo + i
        c = int(np.searchsorted(offs, site, side="right")) - 1
        dm, dsd, lm, lsd = site_summary_row(summary["n_rows"][i], summary["n_samples"][i], summary["dwell_sq"][i], summary["M1"][i],
                                            summary["M2"][i])
        out.append("%s\t%d\t%d\t%d\t%r\t%r\t%r\t%r\n" % (ref_names[c], site - int(offs[c]) + 1, int(summary["n_rows"][i]),
                                                         int(summary["n_samples"][i]), dm, dsd, lm, lsd))
    return out


def write_site_summary(path: str, fetch, num_sites: int, ref_names, offsets, window: int = 1 << 20, quantiles=None) -> int:
    """--site-summary FILE: the header and one line per site with coverage > 0, in reference order. ``fetch(lo, hi)`` returns a
    window of the table (Aligner.site_summary): a genome-sized table is never on the host at once. ``quantiles(lo, hi)``
    (--site-histogram: Aligner.site_quantiles of SITE_QUANTILE_PROBS over the same window) adds the three columns of
    SITE_QUANTILE_HEADER to every line. Returns the sites written."""
    written = 0
    with open(path, "w") as f:
        f.write(SITE_SUMMARY_HEADER if quantiles is None else SITE_SUMMARY_HEADER[:-1] + "\t" + SITE_QUANTILE_HEADER + "\n")
        for lo in range(0, int(num_sites), window):
            hi = min(lo + window, int(num_sites))
            summary = fetch(lo, hi)
            lines = site_summary_lines(summary, lo, ref_names, offsets)
            if quantiles is not None:
                level = quantiles(lo, hi)["level"]
                covered = np.flatnonzero(summary["n_rows"]).tolist()
                lines = [line[:-1] + "".join("\t%r" % float(v) for v in level[i]) + "\n" for line, i in zip(lines, covered)]
            f.writelines(lines)
            written += len(lines)
    return written


# ---- per-site histograms and quantiles (Aligner.set_site_histogram, dynamont-resquiggle --site-histogram) ----------------------
SITE_QUANTILE_PROBS = (0.25, 0.5, 0.75)
SITE_QUANTILE_HEADER = "level_q25\tlevel_median\tlevel_q75"


def site_quantile_levels(rank, bin, below, in_bin, bins: int, lo: float, hi: float) -> np.ndarray:
    """The level of every (site, probability) from what dyn_aligner_site_quantiles returns: the rank's
    place inside its bin, interpolated over the bin's width w = (hi - lo) / bins,
        lo + ((bin - 1) + (rank - below - 0.5) / in_bin) * w      for an interior bin 1 .. bins,
    -inf for the under counter (bin 0), +inf for the over counter (bin bins + 1), NaN for a site without rows (bin 0xFFFFFFFF).
    float64, the shape of ``bin``."""
    b = np.asarray(bin, dtype=np.int64)
    r, bl, ib = (np.asarray(v, dtype=np.float64) for v in (rank, below, in_bin))
    w = (float(hi) - float(lo)) / int(bins)
    out = np.full(b.shape, np.nan, dtype=np.float64)
    inner = (b >= 1) & (b <= int(bins))
    out[inner] = float(lo) + ((b[inner] - 1) + (r[inner] - bl[inner] - 0.5) / ib[inner]) * w
    out[b == 0] = -np.inf
    out[b == int(bins) + 1] = np.inf
    return out


def parse_site_histogram(text: str):
    """--site-histogram BINS[:LO:HI] -> (bins, lo, hi), lo = hi = None when the range is left to the model table
    (site_histogram_range). ValueError for anything else."""
    parts = str(text).split(":")
    try:
        if len(parts) not in (1, 3):
            raise ValueError
        bins = int(parts[0])
        lo, hi = (float(parts[1]), float(parts[2])) if len(parts) == 3 else (None, None)
    except ValueError:
        raise ValueError(f"--site-histogram {text!r}: expected BINS or BINS:LO:HI (an integer and two numbers)") from None
    if not 2 <= bins <= 254:
        raise ValueError(f"--site-histogram {text!r}: BINS must be 2 .. 254")
    if lo is not None and not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"--site-histogram {text!r}: LO and HI must be finite with LO < HI")
    return bins, lo, hi


def site_histogram_range(level_mean, level_stdv):
    """the default range of --site-histogram, from the model table (Aligner.model_table()): four of the widest k-mer's standard
    deviations beyond the lowest and the highest k-mer level"""
    mean, sd = np.asarray(level_mean, dtype=np.float64), np.asarray(level_stdv, dtype=np.float64)
    return float(mean.min() - 4.0 * sd.max()), float(mean.max() + 4.0 * sd.max())
