"""The per-read signal rescaling of Aligner.set_rescale (ABI 10), restated in NumPy: the oracle of the feature.

``rescale_chain`` drives an aligner callable (the CPU oracle, ``oracle.pyoracle.Oracle.align``) pass by pass exactly as
INTEGRATION.md section 3 defines it: align x_k, take the row means y over x_k and the model means m of the rows' k-mers,
fit y = b m + a with sums in chunks of 64 rows, apply the fit when it passes the guards, recompute x_{k+1} from x0.
Every step is one IEEE fp64 operation (NumPy's elementwise and scalar float64 arithmetic, which never contracts)."""
import numpy as np

CHUNK = 64
MIN_ROWS = 16


def chunked_sum(v):
    """sum of v in chunks of 64 consecutive entries: each chunk left to right, the chunk sums left to right"""
    v = np.asarray(v, dtype=np.float64)
    sums = np.array([np.add.accumulate(v[c:c + CHUNK])[-1] for c in range(0, len(v), CHUNK)])
    return np.add.accumulate(sums)[-1]


def segment_means(x, sp):
    """level_mean (ABI 9) of the segments [sp[j], sp[j+1]) of x, the last one up to len(x)"""
    x = np.asarray(x, dtype=np.float64)
    bounds = [int(s) for s in sp] + [len(x)]
    return np.array([chunked_sum(x[a:b]) / np.float64(b - a) for a, b in zip(bounds[:-1], bounds[1:])])


def fit(m, y):
    """(a, b, applied) of the least-squares fit y = b m + a over the rows"""
    m = np.asarray(m, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    n = len(m)
    if n < MIN_ROWS:
        return np.float64(np.nan), np.float64(np.nan), False
    with np.errstate(all="ignore"):
        dn = np.float64(n)
        mbar = chunked_sum(m) / dn
        ybar = chunked_sum(y) / dn
        dm = m - mbar
        sxx = chunked_sum(dm * dm)
        sxy = chunked_sum(dm * (y - ybar))
        b = sxy / sxx
        a = ybar - b * mbar
    ok = bool(sxx > 0 and np.isfinite(a) and np.isfinite(b) and 0.5 <= b <= 2.0 and abs(a) <= 2.0)
    return a, b, ok


def row_model_means(res, model_mean, kmers, k):
    """m_j: the model level_mean of the k-mer of row j (basepos = column - 1 + k/2)"""
    return model_mean[kmers[np.asarray(res["sequence_positions"], dtype=np.int64) - k // 2]]


def rescale_chain(align, x0, seq, model_mean, kmers, k, iters):
    """Passes 0 .. iters of one read. align(x, seq) returns the oracle's dict or raises RuntimeError(message).
    Returns one record per pass k: x (= x_k), res (None if the read failed), error, and shift / scale / iters_applied
    (A_k, B_k and the fits applied before pass k). The result of a job with K = k iterations is record k."""
    x0 = np.asarray(x0, dtype=np.float64)
    A, B = np.float64(0.0), np.float64(1.0)
    applied = 0
    frozen = False
    x = x0
    passes = []
    for p in range(iters + 1):
        try:
            res, err = align(x, seq), None
        except RuntimeError as e:
            res, err = None, str(e)
        passes.append(dict(x=x, res=res, error=err, shift=A, scale=B, iters_applied=applied))
        if p == iters:
            break
        if res is None or frozen:
            frozen = True
            continue
        a, b, ok = fit(row_model_means(res, model_mean, kmers, k), segment_means(x, res["signal_positions"]))
        if not ok:
            frozen = True
            continue
        A = A + B * a
        B = B * b
        applied += 1
        x = (x0 - A) / B
    return passes


def border_agreement(sp, sp_ref):
    """share of rows whose first sample equals the reference's"""
    sp, sp_ref = np.asarray(sp, dtype=np.int64), np.asarray(sp_ref, dtype=np.int64)
    assert len(sp) == len(sp_ref)
    return float(np.mean(sp == sp_ref)) if len(sp) else 1.0


def levels_of(x, sp):
    """level_mean / level_stdv / level_median (ABI 9) of the segments [sp[i], sp[i+1]) of x, the last one up to len(x)"""
    x = np.asarray(x, dtype=np.float64)
    bounds = [int(s) for s in sp] + [len(x)]
    out = np.zeros((3, len(sp)))
    for i, (a, b) in enumerate(zip(bounds[:-1], bounds[1:])):
        seg = x[a:b]
        L = len(seg)
        mean = chunked_sum(seg) / np.float64(L)
        d = seg - mean
        s = np.sort(seg)
        med = s[L // 2] if L % 2 else (s[L // 2 - 1] + s[L // 2]) / 2.0
        out[:, i] = (mean, np.sqrt(chunked_sum(d * d) / np.float64(L)), med + 0.0)
    return out


# ---- recovery of a distorted read: x -> B x + A, K = 3 ----
# Fixed from the CPU run of tests/test_rescale_host.py (restatement + oracle; 16 reads of 60-200 bases per pore and
# distortion, syn9 model). Measured there: |B_3 - B| <= 0.016 and |A_3 - A| <= 0.018 on every read; the share of rows
# whose border equals the undistorted read's: 0.978-0.985 on average (0.94 at the least) at K = 3, 0.63-0.68 on
# average (0.76 at the most) at K = 0.
DISTORTIONS = [(1.2, 0.3), (0.9, -0.2)]   # (B, A): the aligner sees B x + A
RECOVERY_ITERS = 3
RECOVERY_PARAM_TOL = 0.05                  # |B_K - B| and |A_K - A|, every read
RECOVERY_AGREEMENT = 0.90                  # mean border agreement with the undistorted read: >= at K = 3, < at K = 0


# ---- one pass of the device kernels on one read (tests/test_gpu_rescale_kernels.py) ----
def rescale_pass(x, x0, sp, m, state, failed=False):
    """What k_rescale_fit and k_rescale_apply leave of one read. x: the signal the pass aligned, x0: the preprocessed signal,
    sp: the first sample of every row, m: the rows' model means, state: (A, B, applied, frozen, fitted) on entry.
    Returns (state', y, x'): y is None where the kernel returns before the row means (a failed or frozen read, fewer than
    MIN_ROWS rows), x' is x itself (the same object) unless the fit was applied."""
    A, B, applied, frozen, _ = state
    if failed or frozen or len(m) < MIN_ROWS:
        return (A, B, applied, 1, 0), None, x
    y = segment_means(x[int(sp[0]):], np.asarray(sp, dtype=np.int64) - int(sp[0]))
    a, b, ok = fit(m, y)
    if not ok:
        return (A, B, applied, 1, 0), y, x
    A = np.float64(A) + np.float64(B) * a
    B = np.float64(B) * b
    return (A, B, applied + 1, 0, 1), y, (np.asarray(x0, dtype=np.float64) - A) / B
