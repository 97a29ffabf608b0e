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


def write_site_summary(path: str, fetch, num_sites: int, ref_names, offsets, window: int = 1 << 20, quantiles=None, control=None,
                       mixture=None, windows=None) -> int:
    """--site-summary FILE: the header and one line per site with coverage > 0, in reference order. ``fetch(lo, hi)`` returns a
    window of the table (Aligner.site_summary): a genome-sized table is never on the host at once. ``quantiles(lo, hi)``
    (--site-histogram: Aligner.site_quantiles of SITE_QUANTILE_PROBS over the same window) adds the three columns of
    SITE_QUANTILE_HEADER to every line. ``control(lo, hi)`` (--site-control: ``site_control_columns`` over the same window) returns
    one string per site of the window, the eight columns of SITE_CONTROL_HEADER, added to every line behind the others.
    ``mixture(lo, hi)`` (--site-mixture: ``site_mixture_columns`` over the same window) returns one string per site of the window,
    the columns of SITE_MIXTURE_HEADER -- with a control, of SITE_MIXTURE_CONTROL_HEADER too -- added last. Sites are written when
    the RUN has coverage. ``windows`` (a sparse table: Aligner.site_map_windows at log2(window)): the indices w of the windows
    [w * window, (w + 1) * window) that hold a site, the only ones walked then -- the default walks them all; the lines are the
    same, a window without a site has none. Returns the sites written."""
    written = 0
    starts = range(0, int(num_sites), window) if windows is None else [int(w) * window for w in sorted(windows) if int(w) * window < int(num_sites)]
    with open(path, "w") as f:
        header = SITE_SUMMARY_HEADER if quantiles is None else SITE_SUMMARY_HEADER[:-1] + "\t" + SITE_QUANTILE_HEADER + "\n"
        header = header if control is None else header[:-1] + "\t" + SITE_CONTROL_HEADER + "\n"
        if mixture is not None:
            header = header[:-1] + "\t" + SITE_MIXTURE_HEADER + ("" if control is None else "\t" + SITE_MIXTURE_CONTROL_HEADER) + "\n"
        f.write(header)
        for lo in starts:
            hi = min(lo + window, int(num_sites))
            summary = fetch(lo, hi)
            lines = site_summary_lines(summary, lo, ref_names, offsets)
            if quantiles is not None:
                level = quantiles(lo, hi)["level"]
                covered = np.flatnonzero(summary["n_rows"]).tolist()
                lines = [line[:-1] + "".join("\t%r" % float(v) for v in level[i]) + "\n" for line, i in zip(lines, covered)]
            if control is not None:
                extra = control(lo, hi, summary)
                lines = [line[:-1] + "\t" + extra[i] + "\n" for line, i in zip(lines, np.flatnonzero(summary["n_rows"]).tolist())]
            if mixture is not None:
                extra = mixture(lo, hi)
                lines = [line[:-1] + "\t" + extra[i] + "\n" for line, i in zip(lines, np.flatnonzero(summary["n_rows"]).tolist())]
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


# ---- two samples per site (Aligner.site_compare / site_summary_add, dynamont-resquiggle --site-table-out / --site-control) -----
SITE_CONTROL_HEADER = "control_coverage\tks_d\tks_p\tks_level\tks_side\tdwell_ks_d\twelch_t\twelch_df"
SITE_TABLE_VERSION = 1
SITE_TABLE_LIMBS = ("n_rows", "n_samples", "dwell_sq", "m1_lo", "m1_hi", "m2_lo", "m2_hi")


def site_welch(row_a, row_b):
    """Welch's t and its degrees of freedom (Welch-Satterthwaite) between the event means of two sites, from two rows of table
    integers ``(n_rows, M1, M2)`` (Python ints). Means and UNBIASED variances are formed exactly, as
    fractions: mean = M1 / (n 2^40), var = (M2 / 2^40 - n mean^2) / (n - 1), negative variances taken as 0. t^2 and df are exact
    fractions rounded to a double once; t is the square root of that double with the sign of mean_a - mean_b. (nan, nan) when
    either side has fewer than 2 rows or the standard error is 0."""
    from fractions import Fraction
    import math
    (na, m1a, m2a), (nb, m1b, m2b) = [(int(r[0]), int(r[1]), int(r[2])) for r in (row_a, row_b)]
    if na < 2 or nb < 2:
        return math.nan, math.nan
    sides = []
    for n, m1, m2 in ((na, m1a, m2a), (nb, m1b, m2b)):
        mean = Fraction(m1, n << 40)
        var = max(Fraction(0), (Fraction(m2, 1 << 40) - n * mean * mean) / (n - 1))
        sides.append((mean, var / n, n))
    (ma, sa, _), (mb, sb, _) = sides
    se2 = sa + sb
    if se2 == 0:
        return math.nan, math.nan
    diff = ma - mb
    t = math.sqrt(float(diff * diff / se2))
    df = float(se2 * se2 / (sa * sa / (na - 1) + sb * sb / (nb - 1)))
    return (-t if diff < 0 else t), df


def ks_two_sample_p(d: float, n_a: int, n_b: int) -> float:
    """The asymptotic Kolmogorov tail of a two-sample statistic ``d``: ne = n_a n_b / (n_a + n_b),
    lam = (sqrt(ne) + 0.12 + 0.11 / sqrt(ne)) * d, p = 2 sum_{j >= 1} (-1)^(j - 1) exp(-2 j^2 lam^2), summed until a term is below
    1e-16 and clipped to [0, 1]. On BINNED data (``Aligner.site_compare``'s level_d, which never exceeds the distance over the raw
    event means) it is conservative: the p it gives is never below the one the raw samples would give. NaN for a NaN ``d`` or an
    empty side."""
    import math
    if not (n_a > 0 and n_b > 0) or d != d:
        return math.nan
    ne = float(n_a) * float(n_b) / (float(n_a) + float(n_b))
    lam = (math.sqrt(ne) + 0.12 + 0.11 / math.sqrt(ne)) * float(d)
    if lam <= 0.0:
        return 1.0
    if lam < 0.04:     # the series needs 1 / lam terms and its sum is 1 here to within exp(-pi^2 / (8 lam^2)) < 1e-300
        return 1.0
    total, j = 0.0, 1
    while True:
        term = math.exp(-2.0 * j * j * lam * lam)
        total += term if j & 1 else -term
        if term < 1e-16:
            break
        j += 1
    return min(1.0, max(0.0, 2.0 * total))


def save_site_table(path: str, aligner, ref_names, ref_lengths, lo: int = 0, hi=None, window: int = 1 << 20, windows=None,
                    packed: bool = False) -> int:
    """The covered sites of the window [lo, hi) (default: one sample, the references' total length) of ``aligner``'s per-site table
    as an .npz (numpy only): ``site`` uint64 (relative to ``lo``), the seven limb columns, ``level`` / ``dwell`` counters when the
    handle has histograms, ``hist_spec`` = (bins, lo, hi) with the bounds as float64 BITS (uint64; bins 0 = no histograms),
    ``ref_names``, ``ref_lengths``, ``totals`` and ``version``. Fetched window by window: nothing genome-sized is on the host at
    once. ``windows`` (a sparse table: Aligner.site_map_windows at log2(window)): the indices w of the id windows [w * window,
    (w + 1) * window) that hold a site, the only ones fetched then; the file is the same. ``packed``: the covered sites come
    through ``Aligner.site_table_pack`` -- compacted on the GPU, only they cross to the host -- instead of windows of the whole id
    range; the file is the same. Returns the sites saved."""
    lengths = np.asarray(ref_lengths, dtype=np.uint64)
    hi = int(lo) + int(lengths.sum()) if hi is None else int(hi)
    if packed:
        spans = []
    elif windows is None:
        spans = [(w0, min(w0 + int(window), hi)) for w0 in range(int(lo), hi, int(window))]
    else:
        spans = [(max(int(lo), int(w) * int(window)), min(hi, (int(w) + 1) * int(window))) for w in sorted(windows)]
        spans = [(w0, w1) for w0, w1 in spans if w0 < w1]
    spec = getattr(aligner, "_site_histogram", None)
    sites, limbs, level, dwell = [], [[] for _ in SITE_TABLE_LIMBS], [], []
    totals = None
    for w0, w1 in spans:
        t = aligner.site_summary(w0, w1)
        totals = t["totals"]
        idx = np.flatnonzero(t["n_rows"])
        sites.append((idx + (w0 - int(lo))).astype(np.uint64))
        for f in range(7):
            limbs[f].append(np.asarray(t["limbs"][f], dtype=np.uint64)[idx])
        if spec:
            h = aligner.site_histogram(w0, w1)
            level.append(h["level"][idx])
            dwell.append(h["dwell"][idx])
    if packed:
        t = aligner.site_table_pack(int(lo), hi)
        totals = t["totals"]
        idx = np.flatnonzero(t["n_rows"])      # (a live row has a non-zero word; the file keeps the covered ones, as the windows do)
        sites.append(t["site"][idx])
        for f in range(7):
            limbs[f].append(np.asarray(t["limbs"][f], dtype=np.uint64)[idx])
        if spec:
            level.append(t["level"][idx])
            dwell.append(t["dwell"][idx])
    if totals is None:
        totals = aligner.site_summary(int(lo), int(lo))["totals"]
    from dynamont_amd._dynamont import SITE_SUMMARY_TOTALS
    cat = lambda parts, dtype, shape: np.concatenate(parts) if parts else np.zeros(shape, dtype=dtype)  # noqa: E731
    out = {"version": np.array([SITE_TABLE_VERSION], dtype=np.uint32), "num_sites": np.array([hi - int(lo)], dtype=np.uint64),
           "site": cat(sites, np.uint64, 0), "ref_names": np.array([str(n) for n in ref_names], dtype=np.str_), "ref_lengths": lengths,
           "totals": np.array([int(totals[k]) for k in SITE_SUMMARY_TOTALS], dtype=np.uint64)}
    for name, parts in zip(SITE_TABLE_LIMBS, limbs):
        out[name] = cat(parts, np.uint64, 0)
    if spec:
        bins = int(spec[0])
        out["hist_spec"] = np.concatenate([np.array([bins], dtype=np.uint64), np.array(spec[1:], dtype=np.float64).view(np.uint64)])
        out["level"] = cat(level, np.uint32, (0, bins + 2))
        out["dwell"] = cat(dwell, np.uint32, (0, 16))
    else:
        out["hist_spec"] = np.zeros(3, dtype=np.uint64)
    with open(path, "wb") as f:          # (a file object: np.savez appends no extension to the name the caller chose)
        np.savez(f, **out)
    return int(out["site"].size)


def load_site_table(path: str) -> dict:
    """What ``save_site_table`` wrote, as a dict: ``site`` uint64, ``limbs`` (the seven uint64 columns), ``M1`` / ``M2`` (object
    arrays of Python ints), ``level`` / ``dwell`` (None without histograms), ``hist_spec`` = (bins, lo, hi) with float bounds or
    None, ``hist_bits`` (the three uint64 as stored), ``ref_names`` (list of str), ``ref_lengths`` (uint64), ``num_sites``,
    ``totals`` (dict) and ``version``. ValueError for another format version."""
    from dynamont_amd._dynamont import SITE_SUMMARY_TOTALS, int128_of_limbs
    with np.load(path, allow_pickle=False) as z:
        version = int(z["version"][0])
        if version != SITE_TABLE_VERSION:
            raise ValueError(f"{path}: site table format version {version}, this build reads version {SITE_TABLE_VERSION}")
        limbs = [np.ascontiguousarray(z[k], dtype=np.uint64) for k in SITE_TABLE_LIMBS]
        bits = np.asarray(z["hist_spec"], dtype=np.uint64)
        has = int(bits[0]) > 0
        lo, hi = bits[1:].view(np.float64).tolist()
        return {"version": version, "num_sites": int(z["num_sites"][0]), "site": np.asarray(z["site"], dtype=np.uint64), "limbs": limbs,
                "n_rows": limbs[0], "n_samples": limbs[1], "dwell_sq": limbs[2], "M1": int128_of_limbs(limbs[3], limbs[4]),
                "M2": int128_of_limbs(limbs[5], limbs[6]), "level": np.asarray(z["level"], dtype=np.uint32) if has else None,
                "dwell": np.asarray(z["dwell"], dtype=np.uint32) if has else None, "hist_spec": (int(bits[0]), lo, hi) if has else None,
                "hist_bits": bits.copy(), "ref_names": [str(n) for n in z["ref_names"].tolist()],
                "ref_lengths": np.asarray(z["ref_lengths"], dtype=np.uint64),
                "totals": dict(zip(SITE_SUMMARY_TOTALS, [int(v) for v in z["totals"].tolist()]))}


def check_site_control(table: dict, path: str, ref_names, ref_lengths, hist_spec, flag: str = "--site-control") -> None:
    """--site-control: refuses, each with its own message, a saved table whose references differ from the BAM header's in name or
    length, one without histograms, and one whose hist_spec is not bit-equal to the run's ``hist_spec`` = (bins, lo, hi); a bound
    of None (the range left to the model table) is compared once the run knows it. ``flag`` names the option in the messages
    (--site-table-in checks its files the same way); ``hist_spec`` None: the run has no histograms and takes the table alone
    (--site-table-in only: a control always has them)."""
    names, lengths = [str(n) for n in ref_names], [int(v) for v in ref_lengths]
    if table["ref_names"] != names:
        raise ValueError(f"{flag} {path}: its reference names differ from the BAM header's")
    if [int(v) for v in table["ref_lengths"].tolist()] != lengths:
        raise ValueError(f"{flag} {path}: its reference lengths differ from the BAM header's")
    if hist_spec is None:
        return
    if table["hist_spec"] is None:
        raise ValueError(f"{flag} {path}: the file holds no histograms (it was saved by a run without --site-histogram)")
    bins, lo, hi = hist_spec
    mine = [int(bins)] + [None if v is None else int(np.array([v], dtype=np.float64).view(np.uint64)[0]) for v in (lo, hi)]
    theirs = [int(v) for v in table["hist_bits"].tolist()]
    if any(m is not None and m != t for m, t in zip(mine, theirs)):
        raise ValueError(f"{flag} {path}: its histograms ({table['hist_spec'][0]} bins over [{table['hist_spec'][1]!r}, "
                         f"{table['hist_spec'][2]!r})) are not the run's ({bins} bins over [{lo!r}, {hi!r})), bit for bit")


SITE_MODEL_VERSION = 1
SITE_MODEL_COLUMNS = ("pi1", "mu0", "mu1", "var0", "var1")


def save_site_model(path: str, model: dict, ref_names, ref_lengths, histogram=None) -> int:
    """The SET rows (var0 > 0, mu0 and var0 finite) of a per-site model -- the five float64 columns ``pi1``, ``mu0``, ``mu1``,
    ``var0``, ``var1`` over the sites [0, n), as ``Aligner.site_model()`` returns them or ``Aligner.site_mixture()`` fitted them --
    as a sparse .npz (numpy only): ``site`` uint64, the five columns, ``num_sites``, ``ref_names``, ``ref_lengths``, ``hist_spec`` =
    (bins, lo, hi) of the histograms the model was fitted under with the bounds as float64 BITS (bins 0: not recorded) and
    ``version``. A ``model`` that holds ``site`` (ascending uint64) and ``num_sites`` is taken as sparse already: its columns are
    the rows of those sites (a genome-wide id space is never dense on the host). Returns the rows saved."""
    cols = [np.ascontiguousarray(model[k], dtype=np.float64).reshape(-1) for k in SITE_MODEL_COLUMNS]
    n = cols[0].size
    if any(c.size != n for c in cols):
        raise ValueError("save_site_model: the columns of the model differ in length")
    site = np.arange(n, dtype=np.uint64) if model.get("site") is None else np.ascontiguousarray(model["site"], dtype=np.uint64).reshape(-1)
    if site.size != n:
        raise ValueError("save_site_model: the columns of the model differ in length")
    with np.errstate(invalid="ignore"):
        idx = np.flatnonzero((cols[3] > 0) & np.isfinite(cols[1]) & np.isfinite(cols[3]))
    out = {"version": np.array([SITE_MODEL_VERSION], dtype=np.uint32),
           "num_sites": np.array([n if model.get("site") is None else int(model["num_sites"])], dtype=np.uint64),
           "site": site[idx], "ref_names": np.array([str(r) for r in ref_names], dtype=np.str_),
           "ref_lengths": np.asarray(ref_lengths, dtype=np.uint64)}
    for k, c in zip(SITE_MODEL_COLUMNS, cols):
        out[k] = c[idx]
    if histogram:
        out["hist_spec"] = np.concatenate([np.array([int(histogram[0])], dtype=np.uint64), np.array(histogram[1:], dtype=np.float64).view(np.uint64)])
    else:
        out["hist_spec"] = np.zeros(3, dtype=np.uint64)
    with open(path, "wb") as f:          # (a file object: np.savez appends no extension to the name the caller chose)
        np.savez(f, **out)
    return int(idx.size)


def load_site_model(path: str, ref_names=None, ref_lengths=None) -> dict:
    """What ``save_site_model`` wrote: ``site`` uint64 and the five float64 columns over the set rows, ``num_sites``, ``ref_names``,
    ``ref_lengths``, ``histogram`` = (bins, lo, hi) or None, and ``dense(lo, hi)``: the five columns over the sites [lo, hi) with
    zeros (not set) elsewhere -- what ``Aligner.set_site_model(lo, ...)`` takes. With ``ref_names`` / ``ref_lengths`` (the BAM
    header's) a model fitted over other contigs is refused, as ``check_site_control`` refuses a control. ValueError for another
    format version."""
    with np.load(path, allow_pickle=False) as z:
        version = int(z["version"][0])
        if version != SITE_MODEL_VERSION:
            raise ValueError(f"{path}: site model format version {version}, this build reads version {SITE_MODEL_VERSION}")
        out = {"version": version, "num_sites": int(z["num_sites"][0]), "site": np.asarray(z["site"], dtype=np.uint64),
               "ref_names": [str(r) for r in z["ref_names"].tolist()], "ref_lengths": np.asarray(z["ref_lengths"], dtype=np.uint64)}
        for k in SITE_MODEL_COLUMNS:
            out[k] = np.ascontiguousarray(z[k], dtype=np.float64)
        spec = np.asarray(z["hist_spec"], dtype=np.uint64)
    lo_b, hi_b = spec[1:].view(np.float64).tolist()
    out["histogram"] = (int(spec[0]), lo_b, hi_b) if int(spec[0]) else None
    if ref_names is not None:
        if out["ref_names"] != [str(r) for r in ref_names] or \
                [int(v) for v in out["ref_lengths"].tolist()] != [int(v) for v in (ref_lengths if ref_lengths is not None else [])]:
            raise ValueError(f"--site-model {path}: the site model was fitted over other contigs than the BAM header's (names or lengths differ)")
    site = out["site"].astype(np.int64)

    def dense(lo: int, hi: int) -> dict:
        a, b = np.searchsorted(site, [int(lo), int(hi)])
        cols = {k: np.zeros(max(0, int(hi) - int(lo)), dtype=np.float64) for k in SITE_MODEL_COLUMNS}
        for k in SITE_MODEL_COLUMNS:
            cols[k][site[a:b] - int(lo)] = out[k][a:b]
        return cols

    out["dense"] = dense
    return out


def upload_site_model(aligner, model: dict, offset: int = 0, window: int = 1 << 20) -> dict:
    """a loaded model (``load_site_model``) into the sites [offset, offset + num_sites) of ``aligner``'s model
    (``Aligner.set_site_model``), a window of sites at a time and only the windows that hold a set row. Returns the summed
    ``{"stored", "dropped"}``."""
    total = {"stored": 0, "dropped": 0}
    site = model["site"].astype(np.int64)
    for w0 in range(0, int(model["num_sites"]), int(window)):
        w1 = min(w0 + int(window), int(model["num_sites"]))
        a, b = np.searchsorted(site, [w0, w1])
        if a == b:
            continue
        got = aligner.set_site_model(int(offset) + w0, model["dense"](w0, w1), accept=None)
        total["stored"] += got["stored"]
        total["dropped"] += got["dropped"]
    return total


def load_site_control(aligner, table: dict, offset: int, window: int = 1 << 20) -> int:
    """adds a loaded table (``load_site_table``) into the sites [offset, offset + num_sites) of ``aligner``'s table and histograms
    (``Aligner.site_summary_add``), a window of sites at a time; its totals are NOT added: the handle's totals stay the run's own.
    Returns the covered sites added."""
    site = table["site"].astype(np.int64)
    bins = table["hist_spec"][0] if table["hist_spec"] else 0
    spec = getattr(aligner, "_site_histogram", None)
    edges = spec[1] + np.arange(spec[0] + 1, dtype=np.float64) * ((spec[2] - spec[1]) / spec[0]) if spec else None
    for w0 in range(0, int(table["num_sites"]), int(window)):
        w1 = min(w0 + int(window), int(table["num_sites"]))
        a, b = np.searchsorted(site, [w0, w1])
        if a == b:
            continue
        rel = site[a:b] - w0
        cols = {}
        for k in ("n_rows", "n_samples", "dwell_sq"):
            cols[k] = np.zeros(w1 - w0, dtype=np.uint64)
            cols[k][rel] = table[k][a:b]
        for k in ("M1", "M2"):
            cols[k] = np.zeros(w1 - w0, dtype=object)
            cols[k][rel] = table[k][a:b]
        hist = None
        if bins:
            hist = {"level": np.zeros((w1 - w0, bins + 2), dtype=np.uint32), "dwell": np.zeros((w1 - w0, 16), dtype=np.uint32), "edges": edges}
            hist["level"][rel] = table["level"][a:b]
            hist["dwell"][rel] = table["dwell"][a:b]
        aligner.site_summary_add(int(offset) + w0, cols, hist)
    return int(site.size)


def merge_site_table(aligner, table: dict, offset: int = 0, totals: bool = False) -> int:
    """adds a loaded table (``load_site_table``) into ``aligner``'s table and histograms BY KEY (``Aligner.site_summary_merge``):
    site s of the file into the site ``offset + s``, only the file's covered sites cross to the device, however they are
    scattered over the id space. ``totals``: the file's five totals are added too (several flow cells of one sample add up); the
    default leaves the handle's totals the run's own, as ``load_site_control`` does. Returns the covered sites added."""
    spec = getattr(aligner, "_site_histogram", None)
    packed = {"site": table["site"], "limbs": table["limbs"], "totals": table["totals"] if totals else None}
    if table["hist_spec"] and spec:
        packed["level"], packed["dwell"] = table["level"], table["dwell"]
        b, h_lo, h_hi = table["hist_spec"]
        packed["edges"] = h_lo + np.arange(b + 1, dtype=np.float64) * ((h_hi - h_lo) / b)
    aligner.site_summary_merge(packed, int(offset))
    return int(np.asarray(table["site"]).size)


def site_control_columns(compare: dict, run: dict, control: dict) -> list:
    """the eight columns of SITE_CONTROL_HEADER for every site of one window, as strings: ``compare`` = Aligner.site_compare(lo, hi,
    N + lo) (A the run, B the control), ``run`` / ``control`` = Aligner.site_summary of [lo, hi) and [N + lo, N + hi). ks_d =
    level_d, ks_p = ks_two_sample_p of it, ks_level = level_edge, ks_side = level_side, dwell_ks_d = dwell_d, welch_t / welch_df =
    site_welch of the two rows (floats as ``repr``)."""
    out = []
    for i in range(len(compare["n_a"])):
        n_a, n_b = int(compare["n_a"][i]), int(compare["n_b"][i])
        if n_a == 0:
            out.append("")      # not written: the run has no coverage here
            continue
        d = float(compare["level_d"][i])
        t, df = site_welch((run["n_rows"][i], run["M1"][i], run["M2"][i]), (control["n_rows"][i], control["M1"][i], control["M2"][i]))
        out.append("%d\t%r\t%r\t%r\t%d\t%r\t%r\t%r" % (n_b, d, ks_two_sample_p(d, n_a, n_b), float(compare["level_edge"][i]),
                                                         int(compare["level_side"][i]), float(compare["dwell_d"][i]), t, df))
    return out


# ---- a two-component mixture per site (Aligner.site_mixture, dynamont-resquiggle --site-mixture) ---------------------------------
SITE_MIXTURE_HEADER = "mix_share\tmix_mu0\tmix_mu1\tmix_sd0\tmix_sd1\tmix_iters\tmix_status"
SITE_MIXTURE_CONTROL_HEADER = "mix_control_share\tmix_delta\tmix_lor\tmix_p"


def site_mixture_test(r_a: float, n_a: int, r_b: float, n_b: int):
    """(log odds ratio, p) of the soft 2 x 2 table [[r_a, n_a - r_a], [r_b, n_b - r_b]] -- the expected rows of either sample in the
    upper and in the lower component. The log odds ratio adds 0.5 to each cell (Haldane-Anscombe). p is the upper tail of
    Pearson's chi-square of the table as it stands, chi2 = n (r_a (n_b - r_b) - r_b (n_a - r_a))^2 / (n_a n_b k1 k0) with k1 = r_a +
    r_b, k0 = n - k1, one degree of freedom: erfc(sqrt(chi2 / 2)); 1.0 where a margin is 0. The cells are expectations, not counts:
    p is a screening figure. (nan, nan) for a NaN cell."""
    import math
    r_a, r_b, n_a, n_b = float(r_a), float(r_b), float(n_a), float(n_b)
    if r_a != r_a or r_b != r_b:
        return math.nan, math.nan
    c_a, c_b = max(n_a - r_a, 0.0), max(n_b - r_b, 0.0)
    lor = math.log(((r_a + 0.5) * (c_b + 0.5)) / ((c_a + 0.5) * (r_b + 0.5)))
    k1, k0 = r_a + r_b, c_a + c_b
    margins = n_a * n_b * k1 * k0
    if not margins > 0.0:
        return lor, 1.0
    det = r_a * c_b - r_b * c_a
    chi2 = (n_a + n_b) * det * det / margins
    return lor, math.erfc(math.sqrt(chi2 / 2.0))


def site_mixture_columns(mix: dict, control: bool = False) -> list:
    """the columns of SITE_MIXTURE_HEADER for every site of one window, as strings (floats as ``repr``): ``mix`` =
    Aligner.site_mixture(lo, hi) of the run alone, or, with ``control``, Aligner.site_mixture(lo, hi, N + lo) (A the run, B the
    control, pooled), which adds the columns of SITE_MIXTURE_CONTROL_HEADER: mix_share = share_a, mix_control_share = share_b,
    mix_delta their difference, mix_lor / mix_p = site_mixture_test of the soft table. A site without a fit (status 1) prints nan."""
    out = []
    for i in range(len(mix["status"])):
        line = "%r\t%r\t%r\t%r\t%r\t%d\t%d" % (float(mix["share_a"][i]), float(mix["mu0"][i]), float(mix["mu1"][i]), float(mix["sd0"][i]),
                                                float(mix["sd1"][i]), int(mix["iters"][i]), int(mix["status"][i]))
        if control:
            sa, sb = float(mix["share_a"][i]), float(mix["share_b"][i])
            lor, p = site_mixture_test(mix["r_a"][i], mix["n_a"][i], mix["r_b"][i], mix["n_b"][i])
            line += "\t%r\t%r\t%r\t%r" % (sb, sa - sb, lor, p)
        out.append(line)
    return out
