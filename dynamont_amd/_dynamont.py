"""Host-side mirror of the reference's pybind11 module ``dynamont._dynamont``
(src/cpp/aligner_bindings.cpp:180-219), backed by the C ABI in include/dynamont_mi.h.

Same names, argument meaning, return dicts and exception types/messages:

    Aligner(model_file, pore, mode="basic", threads=1, band=400)
    Aligner.align(signal, sequence, calc_probabilities=False) -> dict
    Aligner.train(signal, sequence) -> dict
    PoreType, pore_type(str)

Additions for the GPU (a single read cannot fill an MI355X): ``align_batch``/``train_batch``
and the staged ``Batch`` whose inputs are HBM-resident before kernels run.
"""
from __future__ import annotations

import ctypes as C
import enum
from typing import NamedTuple, Sequence

import numpy as np

from . import _native as N

ERRCAP = 4096


class PoreType(enum.IntEnum):
    """aligner_bindings.cpp:184-189 / include/dynamont/aligner.hpp:26-33"""
    RNA002 = 0
    RNA004 = 1
    DNA_R9 = 2
    DNA_R10_260 = 3
    DNA_R10_400 = 4


def _raise(code: int, msg: str):
    if code == N.DYN_ERR_INVALID_ARGUMENT:
        raise ValueError(msg)          # std::invalid_argument under pybind11
    if code == N.DYN_ERR_OUT_OF_MEMORY:
        raise MemoryError(msg)
    raise RuntimeError(msg)            # std::runtime_error under pybind11 / device failures


def pore_type(pore: str) -> PoreType:
    """aligner_bindings.cpp:18-32,218"""
    out = C.c_int()
    err = C.create_string_buffer(ERRCAP)
    rc = N.lib().dyn_pore_from_string(str(pore).encode(), C.byref(out), err, ERRCAP)
    if rc != N.DYN_OK:
        _raise(rc, err.value.decode())
    return PoreType(out.value)


def read_error_message(status: int, bad_char: bytes | int = 0) -> str:
    buf = C.create_string_buffer(256)
    if isinstance(bad_char, int):
        bad_char = bytes([bad_char & 0xFF])
    N.lib().dyn_read_strerror(int(status), bad_char[:1] or b"\0", buf, 256)
    return buf.value.decode(errors="replace")


def _ptr(a: np.ndarray, t):
    return a.ctypes.data_as(t)


def _pack(signals: Sequence, sequences: Sequence[str]):
    n = len(signals)
    if n != len(sequences):
        raise ValueError("signals and sequences differ in length")
    sig_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    arrs = []
    for i, s in enumerate(signals):
        a = np.ascontiguousarray(s, dtype=np.float64)  # py::array::c_style | forcecast
        if a.ndim != 1:
            raise ValueError("Signal must be a one-dimensional array")  # aligner_bindings.cpp:137-138
        arrs.append(a)
        sig_off[i + 1] = sig_off[i] + a.size
        seq_off[i + 1] = seq_off[i] + len(sequences[i])
    sig = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.float64)
    if sig.size == 0:
        sig = np.zeros(1, dtype=np.float64)[:0]
    seqs = "".join(sequences).encode("latin-1")
    return np.ascontiguousarray(sig), sig_off, seqs, seq_off


class AlignBatchResult:
    """Columnar results of one batch; ``read(i)`` gives the reference's per-read dict."""

    def __init__(self, n, cap):
        self.n = n
        self.cap = cap
        self.Z = np.zeros(n)
        self.status = np.zeros(n, dtype=np.int32)
        self.bad_char = np.zeros(n, dtype=np.uint8)
        self.seg_offsets = np.zeros(n + 1, dtype=np.uint64)
        self.n_segments = np.zeros(n, dtype=np.uint64)
        self.sequence_positions = np.zeros(cap, dtype=np.uint64)
        self.signal_positions = np.zeros(cap, dtype=np.uint64)
        self.probabilities = np.zeros(cap)
        self.states = np.zeros(cap, dtype=np.uint8)
        self._c = N.DynAlignOut(_ptr(self.Z, N.c_double_p), _ptr(self.status, N.c_i32_p),
                                self.bad_char.ctypes.data, _ptr(self.seg_offsets, N.c_u64_p),
                                _ptr(self.n_segments, N.c_u64_p), _ptr(self.sequence_positions, N.c_u64_p),
                                _ptr(self.signal_positions, N.c_u64_p), _ptr(self.probabilities, N.c_double_p),
                                _ptr(self.states, N.c_u8_p), cap)
        # per-segment signal levels (Aligner.set_event_stats): float64 [cap] like the segment columns, None when not requested
        self.level_mean = self.level_stdv = self.level_median = None
        # per-read transforms (Aligner.set_rescale): shift / scale float64 [n], fits applied int32 [n], None when off
        self.rescale_shift = self.rescale_scale = self.rescale_iters = None
        # per-border segment scores (Aligner.set_segment_scores): float64 [cap] like the segment columns, None when off
        self.median_delta = self.mad_delta = self.homogeneity = None
        # per-border posterior confidence (Aligner.set_border_confidence): float64 [cap] like the segment columns, None when off
        self.border_probability = self.border_window_probability = None
        # posterior path samples (Aligner.set_posterior_samples): sample_starts uint32 [K, cap] (sample k of output row s at
        # [k, s]; DYN_SAMPLE_DEAD in every entry of a dead sample), sample_dead uint32 [n]; None when off
        self.sample_starts = self.sample_dead = None
        # per-border credible intervals (Aligner.set_border_interval): border_lo / border_hi uint32 [cap], border_mean / border_sd
        # float64 [cap], indexed like the segment columns; None when off
        self.border_lo = self.border_hi = self.border_mean = self.border_sd = None
        # posterior-weighted per-base sums (Aligner.set_soft_levels): soft_weight / soft_sum / soft_sumsq float64 [cap], indexed
        # like the segment columns; None when off
        self.soft_weight = self.soft_sum = self.soft_sumsq = None
        # per-read site calls (Aligner.set_site_calls): float64 [cap] like the segment columns, NaN = no call; None when off
        self.site_probability = self.site_z = None
        # band-margin diagnostics (Aligner.set_band_margin): uint32 [n] each, None when off; band_used (uint32 [n]): the band
        # every read's rows come from, only with Aligner.set_band_retry
        self.band_margin_low = self.band_margin_high = self.band_edge_rows = None
        self.guide_rounds = self.guide_converged = self.guides = None  # Aligner.align_batch_auto / align_batch_guided(refine > 1)
        self.band_used = None
        # guide rescue (Aligner.set_guide_rescue): uint8 [n] per-read code (0 not flagged, 1 rescued, 2 no room, 3 the rescue
        # failed), None when off; guide_rounds / guide_converged then hold the rescued reads' counts (0 for every other read)
        self.rescue = None

    def _out_struct(self, name: str):
        """the C out-struct of optional result ``name`` (a key of ``_OPTIONAL``) over this object's arrays"""
        cols, struct, _ = _OPTIONAL[name]
        ptrs = [_ptr(getattr(self, attr), ptype) for (attr, _, _), (_, ptype) in zip(cols, struct._fields_)]
        if name == "samples":
            return struct(*ptrs, self.cap, self.n, self.sample_starts.shape[0])
        return struct(*ptrs, self.n if cols[0][2] == "n" else self.cap)

    def _fetch_one(self, L, handle, aligner: "Aligner", name: str, want) -> None:
        """Optional result ``name`` of the job behind ``handle`` into this object's arrays (allocated on first use), or -- ``want``
        false -- drop what an earlier job left there. ``want`` is the job's ``JobWants`` field: the sample count for "samples"."""
        cols, struct, fetch = _OPTIONAL[name]
        if name == "margins":
            self.band_used = None
        if not want:
            if name != "rescue" or self.rescue is not None:  # (without a rescue the guide counts are an auto-guided job's)
                for attr, _, _ in cols:
                    setattr(self, attr, None)
            return
        shapes = [{"n": (self.n,), "cap": (self.cap,), "Kcap": (int(want), self.cap)}[dim] for _, _, dim in cols]
        first = getattr(self, cols[0][0])
        # (the sample planes are reallocated when K changes; a rescue's arrays are fresh every time: the guide counts are shared)
        if first is None or first.shape != shapes[0] or name == "rescue":
            for (attr, dtype, _), shape in zip(cols, shapes):
                setattr(self, attr, np.zeros(shape, dtype=dtype))
        if struct is None:  # dyn_batch_fetch_rescue takes its three arrays as they are
            rc = getattr(L, fetch)(handle, _ptr(self.rescue, N.c_u8_p), _ptr(self.guide_rounds, N.c_u32_p),
                                   _ptr(self.guide_converged, N.c_u32_p), self.n)
        else:
            rc = getattr(L, fetch)(handle, C.byref(self._out_struct(name)))
        if rc != N.DYN_OK:
            _raise(rc, aligner.last_error())

    def _fetch_optional(self, L, handle, aligner: "Aligner", wants: "JobWants") -> None:
        """every optional result of a completed align job, in the order of ``_OPTIONAL``: fetched where ``wants`` says the job
        computed it, dropped where it did not"""
        for name in _OPTIONAL:
            self._fetch_one(L, handle, aligner, name, getattr(wants, name))

    def error(self, i: int) -> str | None:
        if self.status[i] == 0:
            return None
        return read_error_message(int(self.status[i]), int(self.bad_char[i]))

    def read(self, i: int) -> dict:
        """Per-read dict exactly as resultToPython builds it (aligner_bindings.cpp:53-84);
        raises RuntimeError(message) for a failed read like the reference's align()."""
        if self.status[i] != 0:
            raise RuntimeError(self.error(i))
        a = int(self.seg_offsets[i])
        b = a + int(self.n_segments[i])
        d = {
            "Z": float(self.Z[i]),
            "sequence_positions": self.sequence_positions[a:b].copy(),
            "signal_positions": self.signal_positions[a:b].copy(),
            "probabilities": self.probabilities[a:b].copy(),
            "states": [chr(c) for c in self.states[a:b]],
            "polishes": [""] * (b - a),
        }
        if self.level_mean is not None:  # only when requested: the reference's dict is unchanged by default
            d["level_mean"] = self.level_mean[a:b].copy()
            d["level_stdv"] = self.level_stdv[a:b].copy()
            d["level_median"] = self.level_median[a:b].copy()
        if self.median_delta is not None:  # only when requested (Aligner.set_segment_scores)
            d["median_delta"] = self.median_delta[a:b].copy()
            d["mad_delta"] = self.mad_delta[a:b].copy()
            d["homogeneity"] = self.homogeneity[a:b].copy()
        if self.border_probability is not None:  # only when requested (Aligner.set_border_confidence)
            d["border_probability"] = self.border_probability[a:b].copy()
            d["border_window_probability"] = self.border_window_probability[a:b].copy()
        if self.sample_starts is not None:  # only when requested (Aligner.set_posterior_samples): [K, n_segments]
            d["sample_starts"] = self.sample_starts[:, a:b].copy()
        if self.border_lo is not None:  # only when requested (Aligner.set_border_interval)
            for key in ("border_lo", "border_hi", "border_mean", "border_sd"):
                d[key] = getattr(self, key)[a:b].copy()
        if self.soft_weight is not None:  # only when requested (Aligner.set_soft_levels)
            d["soft_dwell"], d["soft_mean"], d["soft_stdv"] = soft_level_columns(self.soft_weight[a:b], self.soft_sum[a:b],
                                                                                 self.soft_sumsq[a:b])
        if self.site_probability is not None:  # only when requested (Aligner.set_site_calls)
            d["site_probability"] = self.site_probability[a:b].copy()
            d["site_z"] = self.site_z[a:b].copy()
        if self.rescale_shift is not None:  # only when requested (Aligner.set_rescale)
            d["rescale_shift"] = float(self.rescale_shift[i])
            d["rescale_scale"] = float(self.rescale_scale[i])
            d["rescale_iters"] = int(self.rescale_iters[i])
        if self.band_margin_low is not None:  # only when requested (Aligner.set_band_margin)
            d["band_margin_low"] = int(self.band_margin_low[i])
            d["band_margin_high"] = int(self.band_margin_high[i])
            d["band_edge_rows"] = int(self.band_edge_rows[i])
        if self.rescue is not None:  # only when requested (Aligner.set_guide_rescue)
            d["rescue"] = int(self.rescue[i])
        return d


def soft_level_columns(weight, total, sumsq):
    """(soft_dwell, soft_mean, soft_stdv) of the three posterior-weighted sums: the weight itself,
    ``sum / weight`` and ``sqrt(max(sumsq / weight - mean^2, 1e-12))`` (the reference's M-step clamp); NaN mean and stdv where the
    weight is 0."""
    w = np.array(weight, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.asarray(total, dtype=np.float64) / w
        var = np.asarray(sumsq, dtype=np.float64) / w - mean * mean
        stdv = np.sqrt(np.where(var < 1e-12, 1e-12, var))
    return w, mean, stdv


class JobWants(NamedTuple):
    """What ONE align job / ticket took of the aligner's opt-in switches at its submission (``Aligner._job_wants``). All off: a
    Z-only or a train job, a batch never aligned."""
    levels: bool = False     # set_event_stats
    rescale: bool = False    # set_rescale
    scores: bool = False     # set_segment_scores
    borders: bool = False    # set_border_confidence
    samples: int = 0         # set_posterior_samples: the count
    intervals: bool = False  # set_border_interval
    margins: bool = False    # set_band_margin (tickets report margins; they are never retried)
    rescue: bool = False     # set_guide_rescue
    soft: bool | None = None  # set_soft_levels (off is None, like the field behind it: both stand behind the positional fields)
    calls: bool | None = None  # set_site_calls (off is None, as for soft)
    auto_guide: tuple | None = None  # set_auto_guide, tickets only: (alignments per read, the ticket's sample offsets)


# the optional results of an align job in the order they are fetched: JobWants field -> ((AlignBatchResult attribute, dtype, one
# entry per read "n" / per segment row "cap" / per sample and segment row "Kcap") in the order of the out-struct's pointers,
# the out-struct, the fetcher)
_F64, _U32 = np.float64, np.uint32
_OPTIONAL = {
    "levels": ((("level_mean", _F64, "cap"), ("level_stdv", _F64, "cap"), ("level_median", _F64, "cap")),
               N.DynEventOut, "dyn_batch_fetch_events"),
    "rescale": ((("rescale_shift", _F64, "n"), ("rescale_scale", _F64, "n"), ("rescale_iters", np.int32, "n")),
                N.DynRescaleOut, "dyn_batch_fetch_rescale"),
    "scores": ((("median_delta", _F64, "cap"), ("mad_delta", _F64, "cap"), ("homogeneity", _F64, "cap")),
               N.DynScoreOut, "dyn_batch_fetch_scores"),
    "borders": ((("border_probability", _F64, "cap"), ("border_window_probability", _F64, "cap")),
                N.DynBorderOut, "dyn_batch_fetch_borders"),
    "samples": ((("sample_starts", _U32, "Kcap"), ("sample_dead", _U32, "n")), N.DynSampleOut, "dyn_batch_fetch_samples"),
    "intervals": ((("border_lo", _U32, "cap"), ("border_hi", _U32, "cap"), ("border_mean", _F64, "cap"), ("border_sd", _F64, "cap")),
                  N.DynBorderIntervalOut, "dyn_batch_fetch_intervals"),
    "soft": ((("soft_weight", _F64, "cap"), ("soft_sum", _F64, "cap"), ("soft_sumsq", _F64, "cap")),
             N.DynSoftLevelOut, "dyn_batch_fetch_soft_levels"),
    "calls": ((("site_probability", _F64, "cap"), ("site_z", _F64, "cap")), N.DynSiteCallOut, "dyn_batch_fetch_site_calls"),
    "margins": ((("band_margin_low", _U32, "n"), ("band_margin_high", _U32, "n"), ("band_edge_rows", _U32, "n")),
                N.DynBandMarginOut, "dyn_batch_fetch_band_margin"),
    "rescue": ((("rescue", np.uint8, "n"), ("guide_rounds", _U32, "n"), ("guide_converged", _U32, "n")),
               None, "dyn_batch_fetch_rescue"),
}


def format_csv(aligner: "Aligner", res: AlignBatchResult, sequences: Sequence[str], readids: Sequence[str],
               signalids: Sequence[str], sig_offsets: Sequence[int], last_index: Sequence[int],
               threads: int = 8, compact: bool = False, seqs_packed=None):
    """Native segmentation_to_string for a batch (dyn_format_csv). Returns (buffer, begin[n], end[n]):
    read i's CSV rows are ``buffer[begin[i]:end[i]]`` (empty for failed reads). ``compact=True`` closes the gaps
    between the reads' ranges (dyn_csv_compact): ``buffer[:end[-1]]`` is then the whole batch in read order.
    ``seqs_packed`` = (bytes, uint64 offsets) of the sequences if the caller already holds them packed."""
    n = res.n
    if seqs_packed is not None:
        seqs, seq_off = seqs_packed
    else:
        seq_off = np.zeros(n + 1, dtype=np.uint64)
        seq_off[1:] = np.cumsum(np.array([len(s) for s in sequences], dtype=np.uint64))
        seqs = "".join(sequences).encode("latin-1")
    rid = (C.c_char_p * n)(*[str(x).encode() for x in readids])
    sid = (C.c_char_p * n)(*[str(x).encode() for x in signalids])
    so = np.ascontiguousarray(sig_offsets, dtype=np.int64)
    li = np.ascontiguousarray(last_index, dtype=np.int64)
    begin = np.zeros(n, dtype=np.uint64)
    end = np.zeros(n, dtype=np.uint64)
    L = N.lib()
    # the optional columns the result carries, in the order the rows hold them: the signal levels (Aligner.set_event_stats), the
    # segment scores (set_segment_scores), the border confidence (set_border_confidence), the posterior samples
    # (set_posterior_samples), the credible intervals (set_border_interval), the soft levels (set_soft_levels), the site calls
    # (set_site_calls)
    ev, sc, bd, sm, bi, sl, ca = (C.byref(res._out_struct(name)) if getattr(res, _OPTIONAL[name][0][0][0]) is not None else None
                                  for name in ("levels", "scores", "borders", "samples", "intervals", "soft", "calls"))
    cap = int(L.dyn_format_csv_bound_calls(aligner._h, n, C.byref(res._c), ev, sc, bd, sm, bi, sl, ca, rid, sid))
    # one grow-only buffer per handle: first-touch page faults of a fresh 350 MB buffer cost ~100x
    # the formatting itself (15 ms per 1 024-read batch with warm pages)
    buf = getattr(aligner, "_csv_buf", None)
    if buf is None or buf.size < cap:
        buf = aligner._csv_buf = np.empty(max(cap, 1), dtype=np.uint8)
    rc = L.dyn_format_csv_calls(aligner._h, n, C.byref(res._c), ev, sc, bd, sm, bi, sl, ca, seqs, _ptr(seq_off, N.c_u64_p), rid, sid,
                          so.ctypes.data_as(C.POINTER(C.c_int64)), li.ctypes.data_as(C.POINTER(C.c_int64)),
                          int(threads), buf.ctypes.data, cap, _ptr(begin, N.c_u64_p), _ptr(end, N.c_u64_p))
    if rc != N.DYN_OK:
        _raise(rc, "dyn_format_csv failed")
    if compact:
        L.dyn_csv_compact(buf.ctypes.data, n, _ptr(begin, N.c_u64_p), _ptr(end, N.c_u64_p))
    return buf, begin, end


class TrainBatchResult:
    def __init__(self, n, cap, num_kmers, pooled: bool, emissions: bool = True):
        """``emissions=False``: no per-read sparse emission updates (their arrays stay empty and the library
        skips the per-column D2H and grouping) -- for jobs that only consume Z, transitions and the pooled
        statistics."""
        if not emissions:
            cap = 0
        self.n = n
        self.num_kmers = num_kmers
        self.Z = np.zeros(n)
        self.status = np.zeros(n, dtype=np.int32)
        self.bad_char = np.zeros(n, dtype=np.uint8)
        self.transitions = np.zeros(3 * n)
        self.em_offsets = np.zeros(n + 1, dtype=np.uint64)
        self.em_count = np.zeros(n, dtype=np.uint64)
        self.em_code = np.zeros(cap, dtype=np.int32)
        self.em_mean = np.zeros(cap)
        self.em_stdev = np.zeros(cap)
        self.em_weight = np.zeros(cap)
        self.em_sum = np.zeros(cap)
        self.em_sumsq = np.zeros(cap)
        self.trans_counts = np.zeros(2 * n)
        self.pooled = np.zeros(3 * num_kmers) if pooled else None
        opt = (lambda a, t: _ptr(a, t)) if emissions else (lambda a, t: None)
        self._c = N.DynTrainOut(_ptr(self.Z, N.c_double_p), _ptr(self.status, N.c_i32_p), self.bad_char.ctypes.data,
                                _ptr(self.transitions, N.c_double_p), _ptr(self.em_offsets, N.c_u64_p),
                                _ptr(self.em_count, N.c_u64_p), opt(self.em_code, N.c_i32_p),
                                opt(self.em_mean, N.c_double_p), opt(self.em_stdev, N.c_double_p),
                                opt(self.em_weight, N.c_double_p), opt(self.em_sum, N.c_double_p),
                                opt(self.em_sumsq, N.c_double_p), _ptr(self.trans_counts, N.c_double_p), cap)

    def error(self, i: int) -> str | None:
        if self.status[i] == 0:
            return None
        return read_error_message(int(self.status[i]), int(self.bad_char[i]))

    def sparse(self, i: int):
        a = int(self.em_offsets[i])
        b = a + int(self.em_count[i])
        return self.em_code[a:b], self.em_mean[a:b], self.em_stdev[a:b]

    def read(self, i: int, model_mean: np.ndarray, model_stdev: np.ndarray) -> dict:
        """Dense dict of trainingResultToPython (aligner_bindings.cpp:86-107), rebuilt on demand."""
        if self.status[i] != 0:
            raise RuntimeError(self.error(i))
        mean = model_mean.copy()
        sd = model_stdev.copy()
        code, m, s = self.sparse(i)
        mean[code] = m
        sd[code] = s
        t = self.transitions[3 * i:3 * i + 3]
        return {
            "Z": float(self.Z[i]),
            "transition_params": {"m1": float(t[0]), "e1": float(t[1]), "e2": float(t[2])},
            "emission_model": [{"mean": float(a), "stdev": float(b)} for a, b in zip(mean, sd)],
        }


def _fetch_into(fetcher: str):
    """the Batch / AsyncBatch method that calls ``fetcher`` (a dyn_batch_fetch_* of an optional result) on caller-owned arrays"""
    def fetch(self, out) -> None:
        rc = getattr(self._L, fetcher)(self._h, C.byref(out))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
    fetch.__doc__ = fetcher + " into caller-owned arrays (raises ValueError for a batch that did not ask)."
    return fetch


class Batch:
    """Staged form (dyn_batch_*): inputs are validated, k-mer coded and resident in HBM after
    construction; align()/train() only launch kernels; fetch() copies results back."""

    _wants = JobWants()  # of the last align(): a batch never aligned has nothing optional to fetch

    def __init__(self, aligner: "Aligner", signals, sig_offsets, seqs: bytes, seq_offsets, raw=None, site_ids=None):
        """raw = None: ``signals`` are normalised float64 samples. raw = dict(shift, scale, window,
        n_sigmas, f32): ``signals`` are RAW float32 / int16 / float64 samples and the preprocessing of
        segment.py:146-153 runs on the device (dyn_batch_create_raw). ``site_ids``: the batch's per-base site ids, packed like
        ``seqs`` (``Aligner.set_site_summary``); kept alive here."""
        self._al = aligner
        self._L = N.lib()
        self.n = len(sig_offsets) - 1
        self._sig_off = np.ascontiguousarray(sig_offsets, dtype=np.uint64)
        self._seq_off = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        self.capacity = int(self._L.dyn_segment_capacity(aligner._h, self.n, _ptr(self._seq_off, N.c_u64_p)))
        h = C.c_void_p()
        if raw is None:
            sig = np.ascontiguousarray(signals, dtype=np.float64)
            self._site_ids = aligner._stage_site_ids(site_ids)
            rc = self._L.dyn_batch_create(aligner._h, self.n, _ptr(sig, N.c_double_p), _ptr(self._sig_off, N.c_u64_p),
                                          seqs, _ptr(self._seq_off, N.c_u64_p), C.byref(h))
        else:
            sig = np.ascontiguousarray(signals)
            code = {np.dtype(np.float32): 0, np.dtype(np.int16): 1, np.dtype(np.float64): 2}.get(sig.dtype)
            if code is None:
                raise ValueError(f"raw signal dtype {sig.dtype} is not float32, int16 or float64")
            shift = np.ascontiguousarray(raw["shift"], dtype=np.float64)
            scale = np.ascontiguousarray(raw["scale"], dtype=np.float64)
            self._site_ids = aligner._stage_site_ids(site_ids)
            rc = self._L.dyn_batch_create_raw(aligner._h, self.n, sig.ctypes.data, code, _ptr(self._sig_off, N.c_u64_p),
                                              _ptr(shift, N.c_double_p), _ptr(scale, N.c_double_p),
                                              int(raw.get("window", 3)), float(raw.get("n_sigmas", 3.0)),
                                              int(bool(raw.get("f32", False))), seqs, _ptr(self._seq_off, N.c_u64_p),
                                              C.byref(h))
        if rc != N.DYN_OK:
            _raise(rc, aligner.last_error())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dyn_batch_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def align(self, calc_probabilities: bool = True) -> None:
        self._wants = self._al._job_wants(calc_probabilities)  # the switches at submission decide what fetch() brings
        rc = self._L.dyn_batch_align(self._h, int(bool(calc_probabilities)))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())

    def set_guide(self, centres, half_width: int) -> None:
        """dyn_batch_set_guide: the next ``align()`` runs every read inside a window of ``half_width`` lattice columns on either
        side of a per-sample guide path. ``centres``: int32, one entry per signal sample of the
        batch in batch order (``dynamont_amd.guide`` builds them); copied to the device before the call returns."""
        g = np.ascontiguousarray(centres, dtype=np.int32)
        if g.ndim != 1:
            raise ValueError("centres must be a one-dimensional int32 array")
        rc = self._L.dyn_batch_set_guide(self._h, _ptr(g, N.c_i32_p), g.size, int(half_width))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())

    def auto_guide(self, half_width: int) -> None:
        """dyn_batch_auto_guide: the library makes the batch's guide itself -- a forward max-plus pre-pass on the device whose
        window of ``half_width`` columns follows the row's best cell -- and installs it as
        ``set_guide`` would. ``guide()`` returns it."""
        rc = self._L.dyn_batch_auto_guide(self._h, int(half_width))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())

    def set_guide_refine(self, max_rounds: int) -> None:
        """dyn_batch_set_guide_refine: the next guided ``align(True)`` re-aligns every read inside the path its last alignment
        called until that path reproduces the guide, ``max_rounds`` (1 .. 64) alignments at the most; 1 = no refinement."""
        rc = self._L.dyn_batch_set_guide_refine(self._h, int(max_rounds))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())

    def guide(self) -> list:
        """dyn_batch_fetch_guide: the batch's current guide as a list of per-read int32 arrays (one entry per sample); after a
        refined alignment every read's guide of its last round"""
        off = (self._sig_off - self._sig_off[0]).astype(np.int64)
        flat = np.zeros(int(off[-1]) if self.n else 0, dtype=np.int32)
        rc = self._L.dyn_batch_fetch_guide(self._h, _ptr(flat, N.c_i32_p), flat.size)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return [flat[int(off[i]):int(off[i + 1])].copy() for i in range(self.n)]

    def guide_rounds(self):
        """dyn_batch_fetch_guide_rounds: (rounds, converged), two uint32 arrays with one entry per read"""
        rounds, conv = np.zeros(self.n, dtype=np.uint32), np.zeros(self.n, dtype=np.uint32)
        rc = self._L.dyn_batch_fetch_guide_rounds(self._h, _ptr(rounds, N.c_u32_p), _ptr(conv, N.c_u32_p), self.n)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return rounds, conv

    def train(self) -> None:
        rc = self._L.dyn_batch_train(self._h)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())

    def train_guided(self) -> None:
        """dyn_batch_train_guided: ``train()`` inside the guide that ``set_guide`` put on the batch (ValueError without one);
        the results are fetched with ``fetch_train`` / ``pooled_device`` as after ``train()``."""
        rc = self._L.dyn_batch_train_guided(self._h)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())

    def fetch(self, out: AlignBatchResult | None = None) -> AlignBatchResult:
        """Results of the last align(). ``out``: a result object of an earlier batch to refill (same
        number of reads, enough segment capacity) instead of allocating and page-faulting in ~50 MB of
        fresh arrays per 1 024-read batch; whatever it held is overwritten."""
        if out is None or out.n != self.n or out.cap < self.capacity:
            out = AlignBatchResult(self.n, self.capacity + self.capacity // 8)
        rc = self._L.dyn_batch_fetch(self._h, C.byref(out._c))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        out._fetch_optional(self._L, self._h, self._al, self._wants)
        return out

    fetch_events = _fetch_into("dyn_batch_fetch_events")              # out: N.DynEventOut
    fetch_scores = _fetch_into("dyn_batch_fetch_scores")              # N.DynScoreOut
    fetch_borders = _fetch_into("dyn_batch_fetch_borders")            # N.DynBorderOut
    fetch_samples = _fetch_into("dyn_batch_fetch_samples")            # N.DynSampleOut
    fetch_intervals = _fetch_into("dyn_batch_fetch_intervals")        # N.DynBorderIntervalOut
    fetch_soft_levels = _fetch_into("dyn_batch_fetch_soft_levels")    # N.DynSoftLevelOut
    fetch_site_calls = _fetch_into("dyn_batch_fetch_site_calls")      # N.DynSiteCallOut
    fetch_band_margin = _fetch_into("dyn_batch_fetch_band_margin")    # N.DynBandMarginOut
    fetch_rescale = _fetch_into("dyn_batch_fetch_rescale")            # N.DynRescaleOut

    def fetch_train(self, pooled: bool = False) -> TrainBatchResult:
        out = TrainBatchResult(self.n, self.capacity, self._al.num_kmers, pooled)
        rc = self._L.dyn_batch_fetch_train(self._h, C.byref(out._c),
                                           _ptr(out.pooled, N.c_double_p) if pooled else None)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return out

    def signals(self) -> np.ndarray:
        """The device-resident (normalised, Hampel-filtered) samples, concatenated."""
        out = np.empty(int(self._sig_off[-1] - self._sig_off[0]))
        rc = self._L.dyn_batch_signals(self._h, _ptr(out, N.c_double_p), out.size)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return out

    def arena_bytes(self) -> int:
        """dyn_batch_arena_bytes: device bytes the last job allocated for per-workgroup lattice arenas (the guided kernel's, or the
        wide-band kernel's); 0 for a batch that took only the paged read queue, and for a Z-only guided job"""
        v = C.c_uint64(0)
        self._L.dyn_batch_arena_bytes(self._h, C.byref(v))
        return int(v.value)

    def timing(self) -> dict:
        t = N.DynTiming()
        self._L.dyn_batch_timing(self._h, C.byref(t))
        return {k: getattr(t, k) for k, _ in N.DynTiming._fields_ if k != "reserved"}

    def device_results(self):
        """(rows_ptr, capacity, state_ptr): device addresses for a gather without a host hop."""
        rows = C.c_void_p()
        st = C.c_void_p()
        cap = C.c_uint64()
        rc = self._L.dyn_batch_device_results(self._h, C.byref(rows), C.byref(cap), C.byref(st))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return rows.value, cap.value, st.value

    def device_pooled(self):
        p = C.c_void_p()
        cnt = C.c_uint64()
        rc = self._L.dyn_batch_device_pooled(self._h, C.byref(p), C.byref(cnt))
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return p.value, cnt.value


class AsyncBatch:
    """Ticket of ``Aligner.align_async`` / ``train_async`` (dyn_batch_align_async): the batch runs on the
    handle's pipeline; ``wait()`` returns the filled result object. The input arrays are kept alive here
    (the library reads them until the batch is complete)."""

    def __init__(self, aligner: "Aligner", handle, result, keep, wants: JobWants):
        self._al = aligner
        self._L = N.lib()
        self._h = handle
        self.result = result
        self._keep = keep
        self._waited = False
        self._wants = wants  # what an align ticket took of the aligner's switches at its submission (a train ticket: all off)
        self._sig_off = wants.auto_guide[1] if wants.auto_guide is not None else None  # what Batch.guide cuts the flat guide at

    def wait(self):
        if not self._waited:
            rc = self._L.dyn_batch_wait(self._h)
            self._waited = True
            if rc != N.DYN_OK:
                _raise(rc, self._al.last_error())
            if isinstance(self.result, AlignBatchResult):
                # a result object refilled from an earlier ticket must not keep that ticket's counts
                self.result.rescue = self.result.guide_rounds = self.result.guide_converged = self.result.guides = None
                self.result._fetch_optional(self._L, self._h, self._al, self._wants)
                if self._wants.auto_guide is not None and self._wants.auto_guide[0] != 1:
                    self.result.guide_rounds, self.result.guide_converged = Batch.guide_rounds(self)
        return self.result

    @property
    def n(self) -> int:
        return self.result.n

    def guide(self) -> list:
        """dyn_batch_fetch_guide on a ticket submitted under ``Aligner.set_auto_guide``: every read's int32 guide of its last
        alignment, one entry per sample (ValueError for a ticket that was not guided)"""
        self.wait()
        if self._wants.auto_guide is None:
            raise ValueError("AsyncBatch.guide: the ticket was submitted without Aligner.set_auto_guide")
        return Batch.guide(self)

    fetch_events = Batch.fetch_events
    fetch_rescale = Batch.fetch_rescale
    fetch_scores = Batch.fetch_scores
    fetch_borders = Batch.fetch_borders
    fetch_samples = Batch.fetch_samples
    fetch_intervals = Batch.fetch_intervals
    fetch_soft_levels = Batch.fetch_soft_levels
    fetch_site_calls = Batch.fetch_site_calls
    fetch_band_margin = Batch.fetch_band_margin

    def timing(self) -> dict:
        self.wait()
        t = N.DynTiming()
        self._L.dyn_batch_timing(self._h, C.byref(t))
        return {k: getattr(t, k) for k, _ in N.DynTiming._fields_}

    device_results = Batch.device_results
    device_pooled = Batch.device_pooled

    def signals(self, count: int) -> np.ndarray:
        """The ticket's device-resident (normalised, Hampel-filtered) samples, concatenated: ``count`` = the number of
        samples submitted. Served after ``wait()`` and before ``close()``, whether or not the launch was shared."""
        self.wait()
        out = np.empty(int(count))
        rc = self._L.dyn_batch_signals(self._h, _ptr(out, N.c_double_p), out.size)
        if rc != N.DYN_OK:
            _raise(rc, self._al.last_error())
        return out

    def close(self):
        if getattr(self, "_h", None):
            self._L.dyn_batch_destroy(self._h)  # waits first if the batch is still in flight
            self._h = None
            self._keep = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def release_cached_memory() -> None:
    """Free the lattice pools that destroyed aligners have parked for their successors (dyn_release_cached_memory)."""
    N.lib().dyn_release_cached_memory()


def pinned_empty(n: int, dtype) -> np.ndarray:
    """An uninitialised 1-D array in page-locked host memory (dyn_host_alloc): H2D/D2H of the asynchronous
    calls then run as plain DMA. The memory is released when the array (and every view of it) is gone."""
    dt = np.dtype(dtype)
    nbytes = max(1, int(n) * dt.itemsize)
    L = N.lib()
    p = L.dyn_host_alloc(nbytes)
    if not p:
        raise MemoryError(f"dyn_host_alloc({nbytes}) failed")

    class _Owner:
        def __init__(self, ptr):
            self.ptr = ptr

        def __del__(self):
            L.dyn_host_free(self.ptr)

    buf = (C.c_char * nbytes).from_address(p)
    buf._owner = _Owner(p)  # ctypes array -> numpy keeps `buf` alive as its base
    return np.frombuffer(buf, dtype=dt, count=int(n))


class _Scattered:
    """A batch's raw slices as a pointer table (DYN_RAW_SCATTERED); keeps the slices alive."""

    def __init__(self, table: np.ndarray, slices, dtype):
        self.table, self.slices, self.dtype = table, slices, np.dtype(dtype)
        self.ctypes = table.ctypes  # .ctypes.data -> the table


KMER_SUMMARY_TOTALS = ("reads_ok", "segments", "samples", "skipped_segments")


def int128_of_limbs(lo, hi) -> np.ndarray:
    """object array of Python ints: the signed 128-bit two's complement values (hi << 64 | lo)"""
    out = np.empty(len(lo), dtype=object)
    for i, (l, h) in enumerate(zip(lo.tolist(), hi.tolist())):
        v = (h << 64) | l
        out[i] = v - (1 << 128) if h >> 63 else v
    return out


def limbs_of_int128(values):
    """the inverse of int128_of_limbs: (lo, hi) uint64 arrays of the 128-bit two's complement of Python ints"""
    v = np.empty(len(values), dtype=object)
    v[:] = [int(x) for x in values]
    if not len(v):
        return np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
    return (v & 0xFFFFFFFFFFFFFFFF).astype(np.uint64), ((v >> 64) & 0xFFFFFFFFFFFFFFFF).astype(np.uint64)


SITE_SUMMARY_TOTALS = ("reads_ok", "rows_added", "samples_added", "rows_without_site", "rows_skipped")
SITE_MODEL_COLUMNS = ("pi1", "mu0", "mu1", "var0", "var1")  # a row of the per-site model (Aligner.set_site_model)


def site_summary_from_limbs(cols, totals) -> dict:
    """the dict Aligner.site_summary() returns, from the seven uint64 arrays and the five totals of the C interface"""
    cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in cols]
    t = [int(x) for x in np.asarray(totals, dtype=np.uint64).tolist()]
    return {"n_rows": cols[0], "n_samples": cols[1], "dwell_sq": cols[2], "M1": int128_of_limbs(cols[3], cols[4]),
            "M2": int128_of_limbs(cols[5], cols[6]), "limbs": cols, "totals": dict(zip(SITE_SUMMARY_TOTALS, t))}


def kmer_summary_from_limbs(cols, totals) -> dict:
    """the dict Aligner.kmer_summary() returns, from the six uint64 arrays and the four totals of the C interface"""
    cols = [np.ascontiguousarray(c, dtype=np.uint64) for c in cols]
    t = [int(x) for x in np.asarray(totals, dtype=np.uint64).tolist()]
    return {"n_segments": cols[0], "n_samples": cols[1], "Q1": int128_of_limbs(cols[2], cols[3]),
            "Q2": int128_of_limbs(cols[4], cols[5]), "limbs": cols, "totals": dict(zip(KMER_SUMMARY_TOTALS, t))}


class Aligner:
    """Mirror of ``_dynamont.Aligner`` (aligner_bindings.cpp:191-216).

    ``device``: HIP device ordinal (default: current device). ``device=None`` with no GPU raises;
    ``device="host"`` creates a handle for the host-side contract only (model/validation), every
    compute call on it raises RuntimeError -- there is no CPU compute path.
    """

    _event_stats = False  # set_event_stats
    _rescale = 0  # set_rescale
    _segment_scores = 0  # set_segment_scores
    _border_confidence = 0  # set_border_confidence
    _posterior_samples = (0, 0)  # set_posterior_samples: (count, seed)
    _border_interval = 0.0  # set_border_interval: the mass
    _soft_levels = False  # set_soft_levels
    _band_margin = False  # set_band_margin
    _auto_guide = (0, 8)  # set_auto_guide: (half_width, refine)
    _band_retry = None  # set_band_retry: (min_margin, max_band, factor)
    _guide_rescue = (0, 0, 8)  # set_guide_rescue: (min_margin, half_width, refine)
    _kmer_summary = False  # set_kmer_summary
    _site_summary = 0  # set_site_summary: num_sites while on
    _site_capacity = 0  # set_site_summary(capacity=): rows of the sparse table, 0 while the table is dense
    _site_table = 0  # ... and the size of the handle's table (it outlives the switch)
    _site_histogram = None  # set_site_histogram: (bins, lo, hi) of the handle's counters (they outlive the switch too)
    _site_calls = False  # set_site_calls
    _strict = 1  # set_strict
    _model_override = None  # set_model: (mean, stdev)

    def __init__(self, model_file: str, pore, mode: str = "basic", threads: int = 1, band: int = 400,
                 device=None):
        if isinstance(pore, str):
            pore = pore_type(pore)
        elif not isinstance(pore, (PoreType, int, np.integer)):
            raise TypeError("pore must be a PoreType or str")
        self._L = N.lib()
        if device == "host":
            dev = N.DYN_DEVICE_HOST_ONLY
        elif device is None:
            dev = -1
        else:
            dev = int(device)
        h = C.c_void_p()
        err = C.create_string_buffer(ERRCAP)
        rc = self._L.dyn_aligner_create(str(model_file).encode(), int(pore), str(mode).encode(), int(threads),
                                        int(band), dev, C.byref(h), err, ERRCAP)
        if rc != N.DYN_OK:
            _raise(rc, err.value.decode())
        self._h = h
        self._ctor = (str(model_file), int(pore), str(mode), int(threads), device)  # what a retry handle is created with
        self.band = int(band)
        self._retry_handles = {}  # band -> Aligner (set_band_retry)
        info = N.DynInfo()
        self._L.dyn_aligner_info(h, C.byref(info))
        self.info = info
        self.pore = PoreType(info.pore)
        self.rna = bool(info.rna)
        self.kmer_size = int(info.kmer_size)
        self.num_kmers = int(info.num_kmers)
        self._model = None

    def close(self):
        for al in getattr(self, "_retry_handles", {}).values():
            al.close()
        self._retry_handles = {}
        if getattr(self, "_h", None):
            self._L.dyn_aligner_destroy(self._h)
            self._h = None

    __del__ = close

    def last_error(self) -> str:
        return (self._L.dyn_aligner_last_error(self._h) or b"").decode(errors="replace")

    def set_mem_budget(self, nbytes: int) -> None:
        self._L.dyn_aligner_set_mem_budget(self._h, int(nbytes))

    STRICT_MODES = {"off": 0, "ties": 1, "start": 1, "all": 2}  # "start": round 3's name of mode 1

    def set_model(self, mean, stdev) -> None:
        """Replace the model table (k-mer-code order, as model_table() returns it): the aligner then equals one built
        from a model file with these values (dyn_aligner_set_model)."""
        t = np.empty(2 * self.num_kmers)
        t[0::2] = np.asarray(mean, dtype=np.float64)
        t[1::2] = np.asarray(stdev, dtype=np.float64)
        rc = self._L.dyn_aligner_set_model(self._h, _ptr(t, N.c_double_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._model = None  # model_table() reads it back
        self._model_override = (np.array(mean, dtype=np.float64), np.array(stdev, dtype=np.float64))

    def set_strict(self, mode) -> None:
        """dyn_aligner_set_strict: 0/"off" plain arithmetic; 1/"ties" (the default of a new handle) reads that carry a
        structural tie -- two neighbouring columns with the same emission parameters -- go through the kernels that
        reproduce the reference's sums bit for bit; 2/"all" every read."""
        m = self.STRICT_MODES[mode] if isinstance(mode, str) else int(mode)
        rc = self._L.dyn_aligner_set_strict(self._h, m)
        if rc != N.DYN_OK:
            raise ValueError(self.last_error() or "strict mode must be 0 (off), 1 (ties) or 2 (all)")
        self._strict = m

    def set_session_mode(self, enabled: bool, reserved_cus: int = 0) -> None:
        """dyn_aligner_set_session_mode: the resident read queue on / off, and compute units kept free of it (for RCCL's
        kernels, which do not fit beside a resident session)."""
        rc = self._L.dyn_aligner_set_session_mode(self._h, 1 if enabled else 0, int(reserved_cus))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())

    def session_stats(self) -> dict:
        """dyn_aligner_session_stats: totals over the closed sessions of the resident read queue (closes an open one and
        waits for its waves first). ``wave_occupancy`` = busy / lifetime wave-cycles."""
        t = N.DynSessionStats()
        rc = self._L.dyn_aligner_session_stats(self._h, C.byref(t))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        d = {k: getattr(t, k) for k, _ in N.DynSessionStats._fields_}
        d["wave_occupancy"] = d["wave_cycles_busy"] / d["wave_cycles_life"] if d["wave_cycles_life"] else 0.0
        pw = C.c_uint64(0)
        self._L.dyn_aligner_session_page_wait(self._h, C.byref(pw))   # paged sessions: the part of `idle` spent getting pages
        d["wave_cycles_pages"] = int(pw.value)
        sp = (C.c_uint64 * 4)()
        self._L.dyn_aligner_session_idle_split(self._h, sp)   # where the idle share sat: first read, its pages, last turn, longest
        d["wave_cycles_before_first_read"], d["wave_cycles_before_first_read_pages"] = int(sp[0]), int(sp[1])
        d["wave_cycles_last_turn"], d["wave_cycles_longest_last_turn"] = int(sp[2]), int(sp[3])
        return d

    def set_event_stats(self, on: bool) -> None:
        """dyn_aligner_set_event_stats: align(calc_probabilities=True) jobs submitted while on also compute the per-segment
        signal levels (level_mean / level_stdv / level_median of the aligned, normalised signal) on the GPU; results carry
        them as ``AlignBatchResult.level_*`` and ``read(i)`` adds the three keys."""
        rc = self._L.dyn_aligner_set_event_stats(self._h, 1 if on else 0)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._event_stats = bool(on)

    def set_segment_scores(self, window: int) -> None:
        """dyn_aligner_set_segment_scores: align(calc_probabilities=True) jobs submitted while ``window`` (0 .. 256) > 0 also
        compute the per-border segment scores (median_delta / mad_delta over ``window`` samples either side of every border,
        homogeneity of every segment) on the GPU; results carry them as
        ``AlignBatchResult.median_delta`` / ``.mad_delta`` / ``.homogeneity`` and ``read(i)`` adds the three keys."""
        rc = self._L.dyn_aligner_set_segment_scores(self._h, int(window))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._segment_scores = int(window)

    def set_border_confidence(self, window: int) -> None:
        """dyn_aligner_set_border_confidence: align(calc_probabilities=True) jobs submitted while ``window`` (0 .. 256) > 0 also
        compute, from the lattice's own posteriors, how sure every border is: ``border_probability`` (the posterior mass on the
        called border) and ``border_window_probability`` (the mass within ``window`` samples of it).
        Results carry them as ``AlignBatchResult.border_probability`` / ``.border_window_probability`` and ``read(i)`` adds
        the two keys."""
        rc = self._L.dyn_aligner_set_border_confidence(self._h, int(window))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._border_confidence = int(window)

    def set_border_interval(self, mass: float) -> None:
        """dyn_aligner_set_border_interval: align(calc_probabilities=True) jobs submitted while ``mass`` (0.01 .. 0.999) > 0 also
        compute, on the GPU from every read's own lattice, the credible interval and the spread of every segment's start
        (INTEGRATION.md section 3): ``AlignBatchResult.border_lo`` / ``.border_hi`` (uint32 ``[cap]``: the quantiles
        ``(1 - mass) / 2`` and ``1 - (1 - mass) / 2`` of the posterior over the start, signal positions like
        ``signal_positions``) and ``.border_mean`` / ``.border_sd`` (float64 ``[cap]``); ``read(i)`` gains the four keys.
        ``mass = 0`` (the default) is off. A job started with ``set_border_confidence``, ``set_posterior_samples``,
        ``set_auto_guide`` or ``set_guide_rescue`` on as well, or on a guided batch, is refused (ValueError); with
        ``set_rescale`` the values are the last pass's. ``MultiAligner`` has no such switch."""
        rc = self._L.dyn_aligner_set_border_interval(self._h, float(mass))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._border_interval = float(mass)

    def set_soft_levels(self, on: bool) -> None:
        """dyn_aligner_set_soft_levels: align(calc_probabilities=True) jobs submitted while it is on also compute, on the GPU from
        every read's own lattice, the posterior-weighted per-base sums: ``AlignBatchResult.soft_weight``
        (the expected dwell of the base, in samples), ``.soft_sum`` and ``.soft_sumsq`` (float64 ``[cap]``: the signal and its
        square under the same weights -- additive over reads and positions, and summed per k-mer the read's share of ``train()``'s
        ``weight`` / ``sum`` / ``sumsq``); ``read(i)`` gains ``soft_dwell``, ``soft_mean`` and ``soft_stdv``. Off by default. A job
        started with ``set_border_confidence``, ``set_posterior_samples``, ``set_border_interval``, ``set_auto_guide`` or
        ``set_guide_rescue`` on as well, or on a guided batch, is refused (ValueError); with ``set_rescale`` the values are the
        last pass's, over the last pass's signal. ``MultiAligner`` has no such switch."""
        rc = self._L.dyn_aligner_set_soft_levels(self._h, int(bool(on)))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._soft_levels = bool(on)

    def set_posterior_samples(self, count: int, seed: int = 0) -> None:
        """dyn_aligner_set_posterior_samples: align(calc_probabilities=True) jobs submitted while ``count`` (0 .. 64) > 0 also
        draw ``count`` complete alignments of every read from the posterior distribution over alignments, on the GPU from the
        read's own lattice, reproducibly from ``seed`` (0 .. 2^64 - 1) and the read's index in its
        batch. Results carry ``AlignBatchResult.sample_starts`` (uint32 ``[count, cap]``: sample k's start of output row s, a
        signal position like ``signal_positions``; ``DYN_SAMPLE_DEAD`` throughout a dead sample) and ``.sample_dead`` (uint32
        ``[n]``); ``read(i)`` adds ``"sample_starts"`` (``[count, n_segments]``). Not together with ``set_band_retry``
        (ValueError); a job started with ``set_rescale``, ``set_auto_guide`` or ``set_guide_rescue`` on as well, or on a guided
        batch, is refused (ValueError). ``MultiAligner`` has no such switch."""
        if int(count) > 0 and self._band_retry:
            raise ValueError("set_posterior_samples with set_band_retry: a retried read's samples would come from another handle, "
                             "keyed by another index")
        rc = self._L.dyn_aligner_set_posterior_samples(self._h, int(count), int(seed) & 0xFFFFFFFFFFFFFFFF)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._posterior_samples = (int(count), int(seed) & 0xFFFFFFFFFFFFFFFF)

    def set_auto_guide(self, half_width: int, refine: int = 8) -> None:
        """dyn_aligner_set_auto_guide: ``align_async`` / ``align_raw_async`` / ``align_vbz_async`` tickets with
        ``calc_probabilities=True`` submitted while ``half_width`` (1 .. 2046) > 0 are aligned inside a guide the library makes
        itself and refines up to ``refine`` (1 .. 64) alignments per read -- what ``align_batch_auto(signals, sequences,
        half_width, refine)`` computes, bit for bit, in one launch per ticket. The result of ``AsyncBatch.wait()`` then carries
        ``guide_rounds`` / ``guide_converged`` (``None`` with ``refine == 1``) and ``AsyncBatch.guide()`` returns the final
        guides. 0 turns it off. Synchronous batches, Z-only and train tickets and ``MultiAligner`` are untouched; a ticket
        submitted with ``set_rescale`` / ``set_border_confidence`` on as well is refused (ValueError)."""
        rc = self._L.dyn_aligner_set_auto_guide(self._h, int(half_width), int(refine))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._auto_guide = (int(half_width), int(refine))

    def set_guide_rescue(self, min_margin: int, half_width: int, refine: int = 8) -> None:
        """dyn_aligner_set_guide_rescue: while ``half_width`` (1 .. 2046) > 0, ``align_batch`` and the ``align_async`` /
        ``align_raw_async`` / ``align_vbz_async`` tickets with ``calc_probabilities=True`` align every read as usual, take every
        read's band margins against the diagonal band and align again -- inside a guide the library makes itself, refined up to
        ``refine`` (1 .. 64) alignments, as ``align_batch_auto(.., half_width, refine)`` would -- only the ok reads whose
        ``min(band_margin_low, band_margin_high)`` is below ``min_margin`` (>= 0; 0 flags nothing), all on the device within
        the same batch or ticket. Results gain ``rescue`` (uint8 [n]: 0 not flagged, 1 rescued, 2 flagged but its lattice does
        not fit the memory budget, 3 flagged but the rescue failed -- 2 and 3 keep the plain answer) and ``guide_rounds`` /
        ``guide_converged`` (0 for reads that were not rescued); ``read(i)`` gains ``"rescue"``. A read the plain alignment
        failed is not rescued. With ``set_band_margin(True)`` a rescued read reports margins against its guided window.
        ``half_width = 0`` turns it off. Not together with ``set_band_retry`` (ValueError); a job started with ``set_rescale``,
        ``set_border_confidence`` or ``set_auto_guide`` on as well is refused (ValueError). ``MultiAligner`` has no such switch."""
        if int(half_width) > 0 and self._band_retry:
            raise ValueError("set_guide_rescue with set_band_retry: both re-align the reads a margin flags; choose one")
        rc = self._L.dyn_aligner_set_guide_rescue(self._h, int(min_margin), int(half_width), int(refine))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._guide_rescue = (int(min_margin), int(half_width), int(refine)) if int(half_width) > 0 else (0, 0, 8)

    def _job_wants(self, calc_probabilities: bool, sig_off=None) -> JobWants:
        """What an align job submitted NOW takes of the switches. ``sig_off``: the sample offsets of a TICKET (the auto-guide switch
        concerns tickets alone). The Z-only job takes nothing; modes ntk / resquiggle have no samples, intervals, soft levels, rescue
        or guide."""
        if not calc_probabilities:
            return JobWants()
        plain = self._ctor[2] not in ("ntk", "resquiggle")
        return JobWants(levels=bool(self._event_stats), rescale=self._rescale > 0, scores=self._segment_scores > 0,
                        borders=self._border_confidence > 0, samples=self._posterior_samples[0] if plain else 0,
                        intervals=plain and self._border_interval > 0, soft=(plain and self._soft_levels) or None,
                        calls=bool(self._site_calls) or None, margins=bool(self._band_margin),
                        rescue=plain and self._guide_rescue[1] > 0,
                        auto_guide=(self._auto_guide[1], sig_off) if plain and sig_off is not None and self._auto_guide[0] > 0 else None)

    def set_rescale(self, iters: int) -> None:
        """dyn_aligner_set_rescale: align(calc_probabilities=True) jobs submitted while ``iters`` (0 .. 8) > 0 align every
        read 1 + iters times, refitting the read's signal shift and scale on the GPU between the passes (INTEGRATION.md
        section 3); all results are those of the last pass, and results carry ``AlignBatchResult.rescale_*``."""
        rc = self._L.dyn_aligner_set_rescale(self._h, int(iters))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._rescale = int(iters)

    def set_kmer_summary(self, on: bool) -> None:
        """dyn_aligner_set_kmer_summary: while on, every segment of every ok read of the align(calc_probabilities=True) jobs
        submitted on this aligner is added to its k-mer's entry of a per-k-mer summary kept on the GPU as exact integers
        (INTEGRATION.md section 3); ``kmer_summary()`` fetches it, ``reset_kmer_summary()`` zeroes it."""
        if on and self._band_retry:
            raise ValueError("set_kmer_summary with set_band_retry: the retried reads would be summed twice")
        rc = self._L.dyn_aligner_set_kmer_summary(self._h, 1 if on else 0)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._kmer_summary = bool(on)

    def set_site_summary(self, num_sites: int, capacity: int | None = None) -> None:
        """dyn_aligner_set_site_summary: while ``num_sites`` > 0, every output row of every ok read of the
        align(calc_probabilities=True) jobs submitted on this aligner WITH ``site_ids=`` is added to its site's entry of a
        per-site table kept on the GPU as exact integers, 56 bytes per site: coverage, dwell and the
        sums of the reads' event means and of their squares. ``site_ids``: one uint32 per base of every sequence, in aligner
        orientation, packed like the sequences (``dynamont_amd.sites`` builds them from a mapping); ``DYN_SITE_NONE`` = no site.
        ``site_summary()`` fetches the table, ``reset_site_summary()`` zeroes it; 0 turns the switch off and keeps the table;
        another size waits for the tickets in flight and starts a new table. Like ``set_kmer_summary`` it is not combined
        with ``set_band_retry``: the retried reads would be summed twice (ValueError).

        ``capacity`` (dyn_aligner_set_site_summary_sparse): a SPARSE table of ``capacity`` rows behind a hash map on the GPU from
        site id to row, 60 bytes per row; ``num_sites`` then only bounds the ids (anything below 4 294 967 295). Every call
        keeps its meaning in id space and, while ``site_map()["rows_dropped"]`` is 0, returns what a dense table returns. A
        row whose id finds no bucket in a full map is dropped as a whole site; choose ``capacity`` well above the sites a run
        touches. Another capacity, or the other mode, is another size."""
        num_sites = int(num_sites)
        if num_sites < 0:
            raise ValueError("set_site_summary: num_sites must be >= 0")
        if capacity is not None and int(capacity) < 1:
            raise ValueError("set_site_summary: capacity must be None (a dense table) or >= 1")
        capacity = 0 if capacity is None else int(capacity)
        if num_sites and self._band_retry:
            raise ValueError("set_site_summary with set_band_retry: the retried reads would be summed twice")
        if capacity:
            rc = self._L.dyn_aligner_set_site_summary_sparse(self._h, num_sites, capacity)
        else:
            rc = self._L.dyn_aligner_set_site_summary(self._h, num_sites)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._site_summary = num_sites
        if num_sites:
            if (num_sites, capacity) != (self._site_table, self._site_capacity):
                self._site_histogram = None  # another size releases the histograms: set_site_histogram again
            self._site_table = num_sites
            self._site_capacity = capacity

    def site_map(self) -> dict:
        """dyn_aligner_site_map_stats: ``capacity``, ``n_keys``, ``rows_dropped`` (job rows whose id found no bucket; they also
        count in the totals' rows_skipped) and ``sites_dropped`` (the same for ``site_summary_add``) of a sparse table."""
        out = np.zeros(4, dtype=np.uint64)
        rc = self._L.dyn_aligner_site_map_stats(self._h, _ptr(out, N.c_u64_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return {"capacity": int(out[0]), "n_keys": int(out[1]), "rows_dropped": int(out[2]), "sites_dropped": int(out[3])}

    def site_map_keys(self, lo: int = 0, hi: int | None = None) -> np.ndarray:
        """dyn_aligner_site_map_keys: the uint32 keys of the buckets [lo, hi) (default: all) of a sparse table's map;
        0xFFFFFFFF is an empty bucket. For diagnostics."""
        lo = int(lo)
        hi = self._site_capacity if hi is None else int(hi)
        keys = np.zeros(max(0, hi - lo), dtype=np.uint32)
        rc = self._L.dyn_aligner_site_map_keys(self._h, lo, hi, _ptr(keys, N.c_u32_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return keys

    def site_map_windows(self, shift: int = 20) -> np.ndarray:
        """dyn_aligner_site_map_windows: the ascending uint64 indices w of the id windows [w << shift, (w + 1) << shift) that hold
        a key of a sparse table, found on the GPU."""
        shift = int(shift)
        count = np.zeros(1, dtype=np.uint64)
        cap = max(1, ((max(self._site_table, 1) - 1) >> shift) + 1) if 0 <= shift <= 31 else 1
        wins = np.zeros(min(cap, 1 << 22), dtype=np.uint64)
        rc = self._L.dyn_aligner_site_map_windows(self._h, shift, _ptr(wins, N.c_u64_p), wins.size, _ptr(count, N.c_u64_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return wins[: int(count[0])].copy()

    def _stage_site_ids(self, site_ids):
        """dyn_aligner_stage_site_ids for the batch-creating call that follows at once; returns the array to keep alive"""
        if site_ids is None:
            return None
        ids = np.ascontiguousarray(site_ids, dtype=np.uint32)
        if ids.ndim != 1:
            raise ValueError("site_ids must be a one-dimensional uint32 array, one id per base")
        rc = self._L.dyn_aligner_stage_site_ids(self._h, _ptr(ids, N.c_u32_p), ids.size)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return ids

    def reset_site_summary(self) -> None:
        rc = self._L.dyn_aligner_site_summary_reset(self._h)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())

    def site_summary(self, lo: int = 0, hi: int | None = None) -> dict:
        """dyn_aligner_site_summary_fetch: the sites [lo, hi) (default: all) of the table after every job that has completed.
        ``n_rows`` (coverage), ``n_samples``, ``dwell_sq``: uint64 arrays; ``M1``, ``M2``: object arrays of Python ints (the
        signed 128-bit sums of rint(m * 2**40) and rint(m * m * 2**40) over the rows' event means m); ``limbs``: the seven raw
        uint64 arrays as fetched; ``totals``: reads_ok, rows_added, samples_added, rows_without_site, rows_skipped. Fetch when
        the pipeline is dry."""
        lo = int(lo)
        hi = self._site_table if hi is None else int(hi)
        n = max(0, hi - lo)
        cols = [np.zeros(n, dtype=np.uint64) for _ in range(7)]
        totals = np.zeros(5, dtype=np.uint64)
        rc = self._L.dyn_aligner_site_summary_fetch(self._h, lo, hi, *[_ptr(c, N.c_u64_p) for c in cols], _ptr(totals, N.c_u64_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return site_summary_from_limbs(cols, totals)

    def set_site_histogram(self, bins: int, lo: float = 0.0, hi: float = 0.0) -> None:
        """dyn_aligner_set_site_histogram: beside the per-site table (``set_site_summary(num_sites > 0)`` first), a histogram of
        the reads' event means with ``bins`` (2 .. 254) equal bins over [``lo``, ``hi``) plus an under and an over counter, and
        a log2 histogram of the dwell (16 bins), per site, as exact uint32 counters filled in the same pass (INTEGRATION.md
        section 3). ``site_histogram()`` fetches them, ``site_quantiles()`` reduces them to quantiles on the GPU,
        ``reset_site_summary()`` zeroes them with the table. ``bins = 0`` stops the counting and keeps the counters; other
        parameters wait for the tickets in flight and start zeroed counters; ``set_site_summary`` with another size releases
        them."""
        bins = int(bins)
        rc = self._L.dyn_aligner_set_site_histogram(self._h, bins, float(lo), float(hi))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        if bins:
            self._site_histogram = (bins, float(lo), float(hi))

    def _site_window(self, lo, hi):
        lo = int(lo)
        hi = self._site_table if hi is None else int(hi)
        return lo, hi, max(0, hi - lo)

    def site_histogram(self, lo: int = 0, hi: int | None = None) -> dict:
        """dyn_aligner_site_histogram_fetch: the counters of the sites [lo, hi) (default: all). ``level``: uint32 [n, bins + 2]
        (column 0 under, 1 .. bins the bins, bins + 1 over); ``dwell``: uint32 [n, 16] (bin d: 2**d <= L < 2**(d + 1), the last
        one open); ``edges``: float64 [bins + 1], the nominal bin edges lo + i * (hi - lo) / bins; ``bins``, ``lo``, ``hi``."""
        lo, hi, n = self._site_window(lo, hi)
        bins, h_lo, h_hi = self._site_histogram or (0, 0.0, 0.0)
        level = np.zeros((n, bins + 2), dtype=np.uint32)
        dwell = np.zeros((n, 16), dtype=np.uint32)
        rc = self._L.dyn_aligner_site_histogram_fetch(self._h, lo, hi, _ptr(level, N.c_u32_p), _ptr(dwell, N.c_u32_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        edges = h_lo + np.arange(bins + 1, dtype=np.float64) * ((h_hi - h_lo) / bins)
        return {"level": level, "dwell": dwell, "edges": edges, "bins": bins, "lo": h_lo, "hi": h_hi}

    def site_quantiles(self, probs, lo: int = 0, hi: int | None = None) -> dict:
        """dyn_aligner_site_quantiles: per site of [lo, hi) (default: all) and per probability of ``probs`` (1 .. 8 values in
        [0, 1]) the rank k = min(max(ceil(q n), 1), n) among the site's n event means, the level counter ``bin`` that holds the
        k-th smallest, the count ``below`` that counter and the count ``in_bin`` -- found on the GPU; the histograms stay there.
        ``n``: uint32 [n_sites]; ``rank``, ``bin``, ``below``, ``in_bin``: uint32 [n_sites, n_probs]; ``level``: float64
        [n_sites, n_probs], the value interpolated inside the bin (``segmentation.utils.site_quantile_levels``: -inf / +inf for
        the under / over counter, NaN for a site without rows); ``probs``."""
        from dynamont_amd.segmentation.utils import site_quantile_levels
        q = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        if not 1 <= q.size <= 8 or not ((q >= 0.0) & (q <= 1.0)).all():
            raise ValueError("site_quantiles: 1 .. 8 probabilities in [0, 1]")
        lo, hi, n = self._site_window(lo, hi)
        cnt = np.zeros(n, dtype=np.uint32)
        cols = [np.zeros((n, q.size), dtype=np.uint32) for _ in range(4)]
        rc = self._L.dyn_aligner_site_quantiles(self._h, lo, hi, _ptr(q, N.c_double_p), q.size, _ptr(cnt, N.c_u32_p),
                                                *[_ptr(c, N.c_u32_p) for c in cols])
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        bins, h_lo, h_hi = self._site_histogram
        return {"n": cnt, "rank": cols[0], "bin": cols[1], "below": cols[2], "in_bin": cols[3], "probs": q,
                "level": site_quantile_levels(cols[0], cols[1], cols[2], cols[3], bins, h_lo, h_hi)}

    def site_summary_add(self, lo: int, summary: dict, histogram: dict | None = None) -> None:
        """dyn_aligner_site_summary_add: adds a table shaped like ``site_summary()``'s -- ``n_rows``, ``n_samples``, ``dwell_sq``,
        ``M1`` / ``M2`` as Python ints, ``totals`` optional -- into the sites [lo, lo + len(n_rows)) of the device table, and the
        counters of ``histogram`` (shaped like ``site_histogram()``'s) into the histograms, all as exact integers (INTEGRATION.md
        section 3): a table saved by an earlier run back onto the device, or two runs' tables into one. ValueError when
        ``histogram["edges"]`` are not bit-equal to the handle's."""
        lo = int(lo)
        cols = [np.ascontiguousarray(summary[k], dtype=np.uint64).reshape(-1) for k in ("n_rows", "n_samples", "dwell_sq")]
        n = cols[0].size
        for k in ("M1", "M2"):
            cols.extend(limbs_of_int128(summary[k]))
        if any(c.size != n for c in cols):
            raise ValueError("site_summary_add: the columns of the summary differ in length")
        totals = None
        if summary.get("totals") is not None:
            t = summary["totals"]
            totals = np.array([int(t[k]) for k in SITE_SUMMARY_TOTALS] if isinstance(t, dict) else [int(x) for x in t], dtype=np.uint64)
            if totals.size != 5:
                raise ValueError("site_summary_add: five totals")
        level = dwell = None
        if histogram is not None:
            bins, h_lo, h_hi = self._site_histogram or (0, 0.0, 0.0)
            mine = h_lo + np.arange(bins + 1, dtype=np.float64) * ((h_hi - h_lo) / bins) if bins else np.zeros(0)
            edges = np.ascontiguousarray(histogram["edges"], dtype=np.float64)
            if bins and (edges.shape != mine.shape or edges.tobytes() != mine.tobytes()):
                raise ValueError("site_summary_add: the histogram's edges are not the handle's (set_site_histogram%r)" % ((bins, h_lo, h_hi),))
            level = np.ascontiguousarray(histogram["level"], dtype=np.uint32)
            dwell = np.ascontiguousarray(histogram["dwell"], dtype=np.uint32)
            if bins and (level.shape != (n, bins + 2) or dwell.shape != (n, 16)):
                raise ValueError("site_summary_add: level must be [n, bins + 2] and dwell [n, 16] for the summary's n sites")
        rc = self._L.dyn_aligner_site_summary_add(self._h, lo, lo + n, *[_ptr(c, N.c_u64_p) for c in cols],
                                                  None if totals is None else _ptr(totals, N.c_u64_p),
                                                  None if level is None else _ptr(level, N.c_u32_p),
                                                  None if dwell is None else _ptr(dwell, N.c_u32_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())

    def site_table_pack(self, lo: int = 0, hi: int | None = None) -> dict:
        """dyn_aligner_site_pack: the LIVE sites of [lo, hi) (default: all) -- those with any non-zero word in the table or, on a
        handle with histograms, in their counters -- compacted on the GPU, so that only they cross to the host (INTEGRATION.md
        section 3). ``site``: uint64, the ids relative to ``lo``, ascending (a dense and a sparse handle on the same reads return
        equal arrays); ``limbs``, ``n_rows``, ``n_samples``, ``dwell_sq``, ``M1``, ``M2``: as ``site_summary()`` has them, one entry
        per live site; with histograms ``level``, ``dwell``, ``edges``, ``bins`` as ``site_histogram()`` has them; ``totals``.
        The rows of the table are walked 2^20 at a time: host memory is one window's records plus the result. Every window's
        call first waits for the tickets in flight, so the records are the table behind every ticket submitted before; tickets
        submitted from another thread WHILE it runs may show in the later windows and in ``totals`` (fetched last): pack when
        the pipeline is dry."""
        lo, hi, _ = self._site_window(lo, hi)
        spec = self._site_histogram
        B = spec[0] + 2 if spec else 0
        rows = self._site_capacity or None
        row_lo, row_hi = (0, rows) if rows else (lo, hi)
        step = 1 << 20
        cap = 1 << 12
        count = np.zeros(1, dtype=np.uint64)
        sites, cells, levels, dwells = [], [], [], []
        r0 = row_lo
        while True:
            r1 = min(r0 + step, row_hi) if row_hi > r0 else r0
            while True:
                site = np.zeros(cap, dtype=np.uint32)
                cell = np.zeros((cap, 7), dtype=np.uint64)
                level = np.zeros((cap, B), dtype=np.uint32) if spec else None
                dwell = np.zeros((cap, 16), dtype=np.uint32) if spec else None
                rc = self._L.dyn_aligner_site_pack(self._h, r0, r1, lo, hi, cap, _ptr(site, N.c_u32_p), _ptr(cell, N.c_u64_p),
                                                   None if level is None else _ptr(level, N.c_u32_p),
                                                   None if dwell is None else _ptr(dwell, N.c_u32_p), _ptr(count, N.c_u64_p))
                n = int(count[0])
                if rc != N.DYN_OK and n > cap:  # the window holds more: nothing was copied, once more with room for them
                    cap = n
                    continue
                if rc != N.DYN_OK:
                    _raise(rc, self.last_error())
                break
            if n:
                sites.append(site[:n].copy())
                cells.append(cell[:n].copy())
                if spec:
                    levels.append(level[:n].copy())
                    dwells.append(dwell[:n].copy())
            r0 = r1
            if r0 >= row_hi:
                break
        site = np.concatenate(sites) if sites else np.zeros(0, dtype=np.uint32)
        cell = np.concatenate(cells) if cells else np.zeros((0, 7), dtype=np.uint64)
        order = np.argsort(site, kind="stable") if rows else None  # (a sparse table: bucket order -> id order)
        pick = (lambda v: v[order]) if order is not None else (lambda v: v)
        cell = pick(cell)
        out = site_summary_from_limbs([np.ascontiguousarray(cell[:, f]) for f in range(7)], list(self.site_summary(0, 0)["totals"].values()))
        out["site"] = pick(site).astype(np.uint64) - np.uint64(lo)
        if spec:
            bins, h_lo, h_hi = spec
            out["level"] = pick(np.concatenate(levels)) if levels else np.zeros((0, B), dtype=np.uint32)
            out["dwell"] = pick(np.concatenate(dwells)) if dwells else np.zeros((0, 16), dtype=np.uint32)
            out["edges"] = h_lo + np.arange(bins + 1, dtype=np.float64) * ((h_hi - h_lo) / bins)
            out["bins"] = bins
        return out

    def site_summary_merge(self, packed: dict, offset: int = 0) -> None:
        """dyn_aligner_site_summary_merge: adds what ``site_table_pack()`` returned -- of this handle or of another one, another
        process's included -- into the table BY KEY: the record of ``site[i]`` into the site ``site[i] + offset``, as exact
        integers, with its counters when ``packed`` has them, and ``packed["totals"]`` (when there) once. The same id may appear
        any number of times (the records of several ranks concatenated). Checked like ``site_summary_add``: ValueError when
        ``packed["edges"]`` are not bit-equal to the handle's or an id + offset is not below the table's sites; MemoryError,
        with the count, when a sparse table had no bucket for some ids -- the others were added."""
        offset = int(offset)
        if offset < 0:
            raise ValueError("site_summary_merge: offset must be >= 0")
        ids = np.ascontiguousarray(packed["site"]).reshape(-1)
        n = ids.size
        if n and (ids.dtype.kind not in "ui" or int(ids.min()) < 0 or int(ids.max()) >= 0xFFFFFFFF):
            raise ValueError("site_summary_merge: site must hold integer ids below 4294967295")
        site = ids.astype(np.uint32)
        if "limbs" in packed and packed["limbs"] is not None:
            cols = [np.ascontiguousarray(c, dtype=np.uint64).reshape(-1) for c in packed["limbs"]]
        else:
            cols = [np.ascontiguousarray(packed[k], dtype=np.uint64).reshape(-1) for k in ("n_rows", "n_samples", "dwell_sq")]
            for k in ("M1", "M2"):
                cols.extend(limbs_of_int128(packed[k]))
        if len(cols) != 7 or any(c.size != n for c in cols):
            raise ValueError("site_summary_merge: seven columns of one entry per site")
        cells = np.ascontiguousarray(np.stack(cols, axis=1)) if n else np.zeros((0, 7), dtype=np.uint64)
        totals = None
        if packed.get("totals") is not None:
            t = packed["totals"]
            totals = np.array([int(t[k]) for k in SITE_SUMMARY_TOTALS] if isinstance(t, dict) else [int(x) for x in t], dtype=np.uint64)
            if totals.size != 5:
                raise ValueError("site_summary_merge: five totals")
        level = dwell = None
        if packed.get("level") is not None or packed.get("dwell") is not None:
            if packed.get("level") is None or packed.get("dwell") is None:
                raise ValueError("site_summary_merge: level and dwell counters are given together or not at all")
            bins, h_lo, h_hi = self._site_histogram or (0, 0.0, 0.0)
            mine = h_lo + np.arange(bins + 1, dtype=np.float64) * ((h_hi - h_lo) / bins) if bins else np.zeros(0)
            edges = np.ascontiguousarray(packed["edges"], dtype=np.float64)
            if bins and (edges.shape != mine.shape or edges.tobytes() != mine.tobytes()):
                raise ValueError("site_summary_merge: the histogram's edges are not the handle's (set_site_histogram%r)" % ((bins, h_lo, h_hi),))
            level = np.ascontiguousarray(packed["level"], dtype=np.uint32)
            dwell = np.ascontiguousarray(packed["dwell"], dtype=np.uint32)
            if bins and (level.shape != (n, bins + 2) or dwell.shape != (n, 16)):
                raise ValueError("site_summary_merge: level must be [n, bins + 2] and dwell [n, 16] for the n sites")
        rc = self._L.dyn_aligner_site_summary_merge(self._h, n, _ptr(site, N.c_u32_p), offset, _ptr(cells, N.c_u64_p),
                                                    None if totals is None else _ptr(totals, N.c_u64_p),
                                                    None if level is None else _ptr(level, N.c_u32_p),
                                                    None if dwell is None else _ptr(dwell, N.c_u32_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())

    def site_compare(self, lo: int = 0, hi: int | None = None, other_lo: int | None = None) -> dict:
        """dyn_aligner_site_compare: the sites [lo, hi) (default: the first half of the table) against the sites starting at
        ``other_lo`` (default ``num_sites // 2 + lo``: the second sample of a table of 2 N sites whose ids were offset by N), pair
        by pair on the GPU; the histograms stay there. ``n_a``, ``n_b``, ``level_at``, ``dwell_at``: uint32; ``level_num``,
        ``dwell_num``: uint64; ``level_side``, ``dwell_side``: int32. ``level_d`` / ``dwell_d``:
        float64, the binned Kolmogorov-Smirnov statistic num / (n_a * n_b), NaN where either side is empty; ``level_edge``:
        the level at the upper edge of counter ``level_at`` (``lo_h + level_at * w``; +inf for the over counter, NaN where
        ``level_at`` is 0xFFFFFFFF)."""
        half = self._site_table // 2
        lo = int(lo)
        hi = half if hi is None else int(hi)
        other_lo = half + lo if other_lo is None else int(other_lo)
        n = max(0, hi - lo)
        u32 = [np.zeros(n, dtype=np.uint32) for _ in range(4)]
        u64 = [np.zeros(n, dtype=np.uint64) for _ in range(2)]
        i32 = [np.zeros(n, dtype=np.int32) for _ in range(2)]
        rc = self._L.dyn_aligner_site_compare(self._h, lo, hi, other_lo, _ptr(u32[0], N.c_u32_p), _ptr(u32[1], N.c_u32_p),
                                              _ptr(u64[0], N.c_u64_p), _ptr(u32[2], N.c_u32_p), _ptr(i32[0], N.c_i32_p),
                                              _ptr(u64[1], N.c_u64_p), _ptr(u32[3], N.c_u32_p), _ptr(i32[1], N.c_i32_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        bins, h_lo, h_hi = self._site_histogram
        den = u32[0].astype(np.float64) * u32[1].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            level_d = np.where(den > 0, u64[0].astype(np.float64) / den, np.nan)
            dwell_d = np.where(den > 0, u64[1].astype(np.float64) / den, np.nan)
        at = u32[2].astype(np.float64)
        edge = h_lo + at * ((h_hi - h_lo) / bins)
        edge = np.where(u32[2] == 0xFFFFFFFF, np.nan, np.where(u32[2] == bins + 1, np.inf, edge))
        return {"n_a": u32[0], "n_b": u32[1], "level_num": u64[0], "level_at": u32[2], "level_side": i32[0], "dwell_num": u64[1],
                "dwell_at": u32[3], "dwell_side": i32[1], "level_d": level_d, "dwell_d": dwell_d, "level_edge": edge}

    def site_mixture(self, lo: int = 0, hi: int | None = None, other_lo: int | None = None, max_iters: int = 128, tol: float = 1e-3,
                     min_n: int = 8) -> dict:
        """dyn_aligner_site_mixture: per site of [lo, hi) (default: all) a mixture of two Gaussians fitted by EM on the GPU to the
        site's level counters -- pooled with those of the site ``other_lo + i`` when ``other_lo`` is given (a run in [0, N) and its
        control in [N, 2 N): ``site_mixture(0, N, N)``) -- and each side's rows split between the two components; the histograms
        stay on the device. Component 1 is the one with the higher level. From the device, float64:
        ``pi1`` (its weight), ``mu0``, ``mu1``, ``var0``, ``var1``, ``r_a``, ``r_b`` (the expected number of A's / B's in-range rows
        in component 1); uint32: ``n_a``, ``n_b`` (in-range rows), ``out_a``, ``out_b`` (under + over), ``iters``, ``status`` (0
        converged, 1 no fit: fewer than ``min_n`` rows or no spread, the floats are NaN; 2 ``max_iters`` reached; 3 a component
        collapsed). Formed on the host: ``sd0``, ``sd1``; ``share_a`` = r_a / n_a and ``share_b`` = r_b / n_b (NaN where the count
        is 0): the modified share of either sample; ``separation`` = (mu1 - mu0) / sqrt(0.5 * (var0 + var1))."""
        lo = int(lo)
        hi = self._site_table if hi is None else int(hi)
        n = max(0, hi - lo)
        max_iters, min_n = int(max_iters), int(min_n)
        if not (0 <= max_iters <= 0xFFFFFFFF and 0 <= min_n <= 0xFFFFFFFF):
            raise ValueError("site_mixture: max_iters and min_n must be non-negative 32-bit integers")
        if other_lo is not None and not 0 <= int(other_lo) < 0xFFFFFFFFFFFFFFFF:
            raise ValueError("site_mixture: other_lo must be a site of the table or None")
        f64 = [np.zeros(n, dtype=np.float64) for _ in range(7)]
        u32 = [np.zeros(n, dtype=np.uint32) for _ in range(6)]
        rc = self._L.dyn_aligner_site_mixture(self._h, lo, hi, 0xFFFFFFFFFFFFFFFF if other_lo is None else int(other_lo), max_iters,
                                              float(tol), min_n, *[_ptr(c, N.c_double_p) for c in f64], *[_ptr(c, N.c_u32_p) for c in u32])
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        out = dict(zip(("pi1", "mu0", "mu1", "var0", "var1", "r_a", "r_b"), f64))
        out.update(zip(("n_a", "n_b", "out_a", "out_b", "iters", "status"), u32))
        with np.errstate(divide="ignore", invalid="ignore"):
            out["sd0"], out["sd1"] = np.sqrt(out["var0"]), np.sqrt(out["var1"])
            out["share_a"] = np.where(out["n_a"] > 0, out["r_a"] / out["n_a"].astype(np.float64), np.nan)
            out["share_b"] = np.where(out["n_b"] > 0, out["r_b"] / out["n_b"].astype(np.float64), np.nan)
            out["separation"] = (out["mu1"] - out["mu0"]) / np.sqrt(0.5 * (out["var0"] + out["var1"]))
        return out

    def set_site_model(self, lo: int, m: dict, accept=(0, 2)) -> dict:
        """dyn_aligner_set_site_model: the dict ``site_mixture()`` returns as the per-site model of the sites [lo, lo + len) -- ``pi1``,
        ``mu0``, ``mu1``, ``var0``, ``var1`` go to the device unchanged for the rows whose ``status`` is in ``accept`` (default:
        converged, or ``max_iters`` reached); every other row is stored NOT SET (five zeros). A dict without ``status`` stores
        every row as it is. The model lives beside the per-site table (``set_site_summary`` first), 40 bytes per table row
        (INTEGRATION.md section 3). Returns ``{"stored": rows sent as set, "dropped": those of them whose id found no bucket in a
        sparse table's map}``."""
        cols = [np.array(m[k], dtype=np.float64).reshape(-1) for k in SITE_MODEL_COLUMNS]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("set_site_model: the columns of the model differ in length")
        if m.get("status") is not None:
            keep = np.isin(np.asarray(m["status"]).reshape(-1), list(accept))
            if keep.size != n:
                raise ValueError("set_site_model: status and the columns of the model differ in length")
            for c in cols:
                c[~keep] = 0.0
        with np.errstate(invalid="ignore"):
            stored = int(((cols[3] > 0) & np.isfinite(cols[1]) & np.isfinite(cols[3])).sum())
        dropped = np.zeros(1, dtype=np.uint64)
        rc = self._L.dyn_aligner_set_site_model(self._h, int(lo), n, *[_ptr(c, N.c_double_p) for c in cols], _ptr(dropped, N.c_u64_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return {"stored": stored, "dropped": int(dropped[0])}

    def site_model(self, lo: int = 0, hi: int | None = None) -> dict:
        """dyn_aligner_site_model_fetch: the model rows of the sites [lo, hi) (default: all) as float64 arrays ``pi1``, ``mu0``,
        ``mu1``, ``var0``, ``var1``; a row that is not set, and an id without a bucket in a sparse table, reads as zeros."""
        lo, hi, n = self._site_window(lo, hi)
        cols = [np.zeros(n, dtype=np.float64) for _ in SITE_MODEL_COLUMNS]
        rc = self._L.dyn_aligner_site_model_fetch(self._h, lo, hi, *[_ptr(c, N.c_double_p) for c in cols])
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return dict(zip(SITE_MODEL_COLUMNS, cols))

    def reset_site_model(self) -> None:
        rc = self._L.dyn_aligner_site_model_reset(self._h)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())

    def set_site_calls(self, on: bool) -> None:
        """dyn_aligner_set_site_calls: align(calc_probabilities=True) jobs submitted while on also score every output row against
        the per-site model (``set_site_model``) on the GPU: ``AlignBatchResult.site_z``, the row's event mean as a z-score under
        the site's component 0, and ``site_probability``, the posterior probability of component 1 of the site's mixture
        (INTEGRATION.md section 3); NaN where there is no call -- no id, no model row, a one-component row (``site_z`` alone).
        Needs ``set_site_summary`` on and ``site_ids=`` with the job; jobs of any other kind are refused while it is on."""
        rc = self._L.dyn_aligner_set_site_calls(self._h, 1 if on else 0)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._site_calls = bool(on)

    def set_band_margin(self, on: bool) -> None:
        """dyn_aligner_set_band_margin: align(calc_probabilities=True) jobs submitted while on also report, per read, how
        close the called path came to a real edge of its band: ``AlignBatchResult.band_margin_low``
        / ``.band_margin_high`` (uint32 [n], ``DYN_BAND_MARGIN_NONE`` = 0xFFFFFFFF where that edge was never a real one) and
        ``.band_edge_rows`` (path rows on a real edge); ``read(i)`` adds the three keys. A margin of 0 says that the band may
        have decided the alignment."""
        rc = self._L.dyn_aligner_set_band_margin(self._h, 1 if on else 0)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        self._band_margin = bool(on)

    def set_band_retry(self, min_margin: int, max_band: int = 4093, factor: int = 2) -> None:
        """The synchronous ``align_batch`` aligns every ok read whose ``min(band_margin_low, band_margin_high)`` is below
        ``min_margin`` again at the band ``min(band * factor, max_band)``, on a second handle with this one's model, pore,
        device and settings, and repeats until the margin passes or ``max_band`` is reached. A read's row count does not
        depend on the band: the new rows, Z, margins and every opt-in column that is on replace the read's entries of the
        first result in place, and ``band_used`` (uint32 [n]) records the band each read's rows come from. A read whose
        retry fails keeps its last good result. Implies ``set_band_margin(True)``; ``min_margin = 0`` turns the retry off
        (the margins stay on). ``align_async`` tickets report margins but are never retried. Not together with
        ``set_kmer_summary(True)`` or ``set_site_summary(num_sites > 0)``: the retried reads would be summed twice (ValueError)."""
        min_margin, max_band, factor = int(min_margin), int(max_band), int(factor)
        if min_margin < 0 or factor < 2 or max_band < 1:
            raise ValueError("set_band_retry: min_margin >= 0, factor >= 2 and max_band >= 1 are required")
        if min_margin == 0:
            self._band_retry = None
            return
        if self._guide_rescue[1] > 0:
            raise ValueError("set_band_retry with set_guide_rescue: both re-align the reads a margin flags; choose one")
        if self._kmer_summary:
            raise ValueError("set_band_retry with set_kmer_summary: the retried reads would be summed twice")
        if self._site_summary:
            raise ValueError("set_band_retry with set_site_summary: the retried reads would be summed twice")
        if self._posterior_samples[0] > 0:
            raise ValueError("set_band_retry with set_posterior_samples: a retried read's samples would come from another handle, "
                             "keyed by another index")
        self.set_band_margin(True)
        self._band_retry = (min_margin, max_band, factor)

    def _retry_handle(self, band: int) -> "Aligner":
        """the handle the retried reads run on at ``band``, with this handle's settings as they stand now"""
        al = self._retry_handles.get(band)
        if al is None:
            model_file, pore, mode, threads, device = self._ctor
            if device is None or device == "host":
                device = int(self.info.device)
            al = self._retry_handles[band] = Aligner(model_file, pore, mode=mode, threads=threads, band=band, device=device)
        if self._model_override is not None:
            al.set_model(*self._model_override)
        al.set_strict(self._strict)
        al.set_event_stats(self._event_stats)
        al.set_rescale(self._rescale)
        al.set_segment_scores(self._segment_scores)
        al.set_border_confidence(self._border_confidence)
        al.set_border_interval(self._border_interval)
        al.set_soft_levels(self._soft_levels)
        al.set_band_margin(True)
        return al

    # per-row and per-read columns a retried read's entries are spliced into (those that are on)
    _ROW_COLUMNS = ("sequence_positions", "signal_positions", "probabilities", "states", "level_mean", "level_stdv", "level_median",
                    "median_delta", "mad_delta", "homogeneity", "border_probability", "border_window_probability",
                    "border_lo", "border_hi", "border_mean", "border_sd", "soft_weight", "soft_sum", "soft_sumsq")
    _READ_COLUMNS = ("Z", "rescale_shift", "rescale_scale", "rescale_iters", "band_margin_low", "band_margin_high", "band_edge_rows")

    def _retry_bands(self, res: AlignBatchResult, signals: Sequence, sequences: Sequence[str]) -> None:
        min_margin, max_band, factor = self._band_retry
        band = self.band
        res.band_used = np.full(res.n, band, dtype=np.uint32)

        def flagged(r, idx):
            m = np.minimum(r.band_margin_low[idx], r.band_margin_high[idx])
            return (r.status[idx] == 0) & (m < min_margin)

        every = np.arange(res.n)
        pending = every[flagged(res, every)]
        while pending.size and band < max_band:
            band = min(band * factor, max_band)
            r2 = self._retry_handle(band).align_batch([signals[i] for i in pending], [sequences[i] for i in pending], True)
            for k, i in enumerate(pending):
                ns = int(res.n_segments[i])
                if r2.status[k] != 0 or int(r2.n_segments[k]) != ns:
                    continue  # the read keeps its last good result
                a, a2 = int(res.seg_offsets[i]), int(r2.seg_offsets[k])
                for name in self._ROW_COLUMNS:
                    col = getattr(res, name)
                    if col is not None:
                        col[a:a + ns] = getattr(r2, name)[a2:a2 + ns]
                for name in self._READ_COLUMNS:
                    col = getattr(res, name)
                    if col is not None:
                        col[i] = getattr(r2, name)[k]
                res.band_used[i] = band
            sub = np.arange(pending.size)
            pending = pending[(r2.status[sub] == 0) & flagged(r2, sub)]

    def reset_kmer_summary(self) -> None:
        rc = self._L.dyn_aligner_kmer_summary_reset(self._h)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())

    def kmer_summary(self) -> dict:
        """dyn_aligner_kmer_summary_fetch: the summary of every job that has completed, in k-mer-code order. ``n_segments``,
        ``n_samples``: uint64 arrays; ``Q1``, ``Q2``: object arrays of Python ints (the signed 128-bit sums of
        rint(S1 * 2**40) and rint(S2 * 2**40) per segment); ``limbs``: the six raw uint64 arrays as fetched; ``totals``:
        reads_ok, segments, samples, skipped_segments. Fetch when the pipeline is dry."""
        n = self.num_kmers
        cols = [np.zeros(n, dtype=np.uint64) for _ in range(6)]
        totals = np.zeros(4, dtype=np.uint64)
        rc = self._L.dyn_aligner_kmer_summary_fetch(self._h, *[_ptr(c, N.c_u64_p) for c in cols], _ptr(totals, N.c_u64_p))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return kmer_summary_from_limbs(cols, totals)

    def set_train_zcheck(self, on: bool) -> None:
        """dyn_aligner_set_train_zcheck: also refuse the reads the reference's |Zf - Zb| rule refuses (one more Z-only
        forward sweep per read)."""
        self._L.dyn_aligner_set_train_zcheck(self._h, 1 if on else 0)

    def tie_rows(self, kmers, signal_len: int) -> int:
        """dyn_tie_rows: 0 = the read carries no structural tie; else the forward rows mode "ties" runs bit for bit
        (0xffffffff = all)."""
        km = np.ascontiguousarray(kmers, dtype=np.int32)
        return int(self._L.dyn_tie_rows(self._h, _ptr(km, N.c_i32_p), len(km), int(signal_len)))

    def model_table(self):
        """(mean, stdev) in k-mer-code order."""
        if self._model is None:
            out = np.zeros(2 * self.num_kmers)
            self._L.dyn_aligner_model(self._h, _ptr(out, N.c_double_p))
            self._model = (out[0::2].copy(), out[1::2].copy())
        return self._model

    # -- host-side contract -------------------------------------------------------------------
    def validate(self, signal_lengths: Sequence[int], sequences: Sequence[str]):
        """validateInput + sequenceToKmers per read: (status[n], messages[n], kmers list)."""
        n = len(sequences)
        sig_off = np.zeros(n + 1, dtype=np.uint64)
        sig_off[1:] = np.cumsum(np.asarray(signal_lengths, dtype=np.uint64))
        seq_off = np.zeros(n + 1, dtype=np.uint64)
        seq_off[1:] = np.cumsum(np.array([len(s) for s in sequences], dtype=np.uint64))
        seqs = "".join(sequences).encode("latin-1")
        status = np.zeros(n, dtype=np.int32)
        bad = np.zeros(n, dtype=np.uint8)
        cap = int(self._L.dyn_segment_capacity(self._h, n, _ptr(seq_off, N.c_u64_p)))
        kmers = np.zeros(max(cap, 1), dtype=np.int32)
        rc = self._L.dyn_validate_batch(self._h, n, _ptr(sig_off, N.c_u64_p), seqs, _ptr(seq_off, N.c_u64_p),
                                        _ptr(status, N.c_i32_p), bad.ctypes.data, _ptr(kmers, N.c_i32_p), cap)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        msgs = [None if s == 0 else read_error_message(int(s), int(b)) for s, b in zip(status, bad)]
        out, off = [], 0
        for i, s in enumerate(sequences):
            kc = max(0, len(s) - self.kmer_size + 1)
            out.append(kmers[off:off + kc].copy() if status[i] == 0 else None)
            off += kc
        return status, msgs, out

    # -- batch API ------------------------------------------------------------------------------
    def batch(self, signals: Sequence, sequences: Sequence[str], site_ids=None) -> Batch:
        """``site_ids``: the batch's per-base uint32 site ids, packed like the sequences (``set_site_summary``)"""
        sig, sig_off, seqs, seq_off = _pack(signals, sequences)
        return Batch(self, sig, sig_off, seqs, seq_off, site_ids=site_ids)

    def batch_packed(self, signals, sig_offsets, seqs: bytes, seq_offsets) -> Batch:
        return Batch(self, signals, sig_offsets, seqs, seq_offsets)

    def batch_raw(self, raw_slices: Sequence, sequences: Sequence[str], shift, scale, window: int = 3,
                  n_sigmas: float = 3.0, f32: bool = False) -> Batch:
        """Batch from RAW sample slices (all float32, all int16 or all float64): normalisation and the
        Hampel filter of the reference's workers run on the device, bit-identically."""
        n = len(raw_slices)
        sig_off = np.zeros(n + 1, dtype=np.uint64)
        seq_off = np.zeros(n + 1, dtype=np.uint64)
        for i, s in enumerate(raw_slices):
            sig_off[i + 1] = sig_off[i] + len(s)
            seq_off[i + 1] = seq_off[i] + len(sequences[i])
        raw = np.concatenate(raw_slices) if n else np.zeros(0, dtype=np.float32)
        seqs = "".join(sequences).encode("latin-1")
        return Batch(self, raw, sig_off, seqs, seq_off,
                     raw=dict(shift=shift, scale=scale, window=window, n_sigmas=n_sigmas, f32=f32))

    def align_async(self, signals, sig_offsets, seqs: bytes, seq_offsets, calc_probabilities: bool = True,
                    out: AlignBatchResult | None = None, site_ids=None) -> AsyncBatch:
        """dyn_batch_align_async on packed inputs (``synth.pack_reads`` layout): returns at once; the batch's
        validation, H2D, kernels, D2H and unpacking overlap with those of the batches submitted around it.
        ``out``: result object of an EARLIER, completed batch to refill. ``site_ids``: the ticket's per-base uint32 site ids,
        packed like ``seqs`` (``set_site_summary``); the ticket keeps the array alive."""
        sig = np.ascontiguousarray(signals, dtype=np.float64)
        sig_off = np.ascontiguousarray(sig_offsets, dtype=np.uint64)
        seq_off = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = len(sig_off) - 1
        cap = int(self._L.dyn_segment_capacity(self._h, n, _ptr(seq_off, N.c_u64_p)))
        if out is None or out.n != n or out.cap < cap:
            out = AlignBatchResult(n, cap + cap // 8)
        h = C.c_void_p()
        ids = self._stage_site_ids(site_ids)
        rc = self._L.dyn_batch_align_async(self._h, n, _ptr(sig, N.c_double_p), _ptr(sig_off, N.c_u64_p), seqs,
                                           _ptr(seq_off, N.c_u64_p), int(bool(calc_probabilities)), C.byref(out._c),
                                           C.byref(h))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return AsyncBatch(self, h, out, (sig, sig_off, seqs, seq_off, ids), wants=self._job_wants(calc_probabilities, sig_off))

    def _raw_args(self, raw, shift, scale, calibration=None):
        scattered = isinstance(raw, (list, tuple))
        if scattered:  # one array per read: the library gathers them (DYN_RAW_SCATTERED), no concatenation here
            slices = [np.ascontiguousarray(x) for x in raw]
            dt = slices[0].dtype if slices else np.dtype(np.int16)
            if any(x.dtype != dt for x in slices):
                raise ValueError("raw slices of one batch must share a dtype")
            table = np.fromiter((x.ctypes.data for x in slices), dtype=np.uint64, count=len(slices))
            raw = _Scattered(table, slices, dt)
        else:
            raw = np.ascontiguousarray(raw)
        code = {np.dtype(np.float32): 0, np.dtype(np.int16): 1, np.dtype(np.float64): 2}.get(raw.dtype)
        if code is None:
            raise ValueError(f"raw signal dtype {raw.dtype} is not float32, int16 or float64")
        if scattered:
            code |= 0x100
        cal = (None, None)
        if calibration is not None:  # int16 ADC + pod5 calibration: picoampere formed on the device
            if code & 0xff != 1:
                raise ValueError("calibration arrays go with int16 ADC samples")
            code = 3 | (code & 0x100)
            cal = (np.ascontiguousarray(calibration[0], dtype=np.float32), np.ascontiguousarray(calibration[1], dtype=np.float32))
        return raw, code, np.ascontiguousarray(shift, dtype=np.float64), np.ascontiguousarray(scale, dtype=np.float64), cal

    def align_raw_async(self, raw, raw_offsets, shift, scale, seqs: bytes, seq_offsets, window: int = 3,
                        n_sigmas: float = 3.0, f32: bool = False, calc_probabilities: bool = True,
                        out: AlignBatchResult | None = None, calibration=None, site_ids=None) -> AsyncBatch:
        """dyn_batch_align_raw_async: ``raw`` = the concatenated RAW [start:end) slices of the batch (float32 pA,
        int16 ADC or float64), or a LIST of per-read arrays (gathered by the library's helper threads, no copy here); normalisation + Hampel filter (segment.py:146-153) run on the device as the first
        stage of the asynchronous pipeline. ``calibration`` = (offset[n], scale[n]) with int16 ``raw``: the samples are
        ADC counts and picoampere = (float32(adc) + offset) * scale is formed on the device too (what pod5's
        ``signal_pa`` computes on the host). Returns at once."""
        raw, code, shift, scale, cal = self._raw_args(raw, shift, scale, calibration)
        raw_off = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        seq_off = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = len(raw_off) - 1
        cap = int(self._L.dyn_segment_capacity(self._h, n, _ptr(seq_off, N.c_u64_p)))
        if out is None or out.n != n or out.cap < cap:
            out = AlignBatchResult(n, cap + cap // 8)
        h = C.c_void_p()
        ids = self._stage_site_ids(site_ids)
        rc = self._L.dyn_batch_align_raw_async(self._h, n, raw.ctypes.data, code, _ptr(raw_off, N.c_u64_p),
                                               _ptr(cal[0], N.c_float_p) if code & 0xff == 3 else None,
                                               _ptr(cal[1], N.c_float_p) if code & 0xff == 3 else None, _ptr(shift, N.c_double_p), _ptr(scale, N.c_double_p), int(window),
                                               float(n_sigmas), int(bool(f32)), seqs, _ptr(seq_off, N.c_u64_p),
                                               int(bool(calc_probabilities)), C.byref(out._c), C.byref(h))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return AsyncBatch(self, h, out, (raw, raw_off, shift, scale, seqs, seq_off, cal, ids),
                          wants=self._job_wants(calc_probabilities, raw_off))

    def align_vbz_async(self, chunks, raw_offsets, shift, scale, seqs: bytes, seq_offsets, window: int = 3,
                        n_sigmas: float = 3.0, f32: bool = False, calc_probabilities: bool = True,
                        out: AlignBatchResult | None = None, calibration=None, site_ids=None) -> AsyncBatch:
        """dyn_batch_align_vbz_async: the batch's signal as POD5 chunks that are still VBZ-compressed. ``chunks`` =
        (ptrs uint64[c], nbytes uint64[c], samples uint32[c], read_chunk_offsets uint64[n+1], slice_start uint64[n]);
        ``raw_offsets`` = prefix sums of the slice lengths. The library's helper threads decode straight into the pinned
        staging buffer."""
        ptrs, nbytes, samples, read_off, skip = (np.ascontiguousarray(x, dtype=d) for x, d in
                                                 zip(chunks, (np.uint64, np.uint64, np.uint32, np.uint64, np.uint64)))
        shift = np.ascontiguousarray(shift, dtype=np.float64)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        cal = (None, None)
        if calibration is not None:
            cal = (np.ascontiguousarray(calibration[0], dtype=np.float32), np.ascontiguousarray(calibration[1], dtype=np.float32))
        raw_off = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        seq_off = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = len(raw_off) - 1
        cap = int(self._L.dyn_segment_capacity(self._h, n, _ptr(seq_off, N.c_u64_p)))
        if out is None or out.n != n or out.cap < cap:
            out = AlignBatchResult(n, cap + cap // 8)
        h = C.c_void_p()
        ids = self._stage_site_ids(site_ids)
        rc = self._L.dyn_batch_align_vbz_async(self._h, n, ptrs.ctypes.data, _ptr(nbytes, N.c_u64_p),
                                               samples.ctypes.data_as(C.POINTER(C.c_uint32)), _ptr(read_off, N.c_u64_p),
                                               _ptr(skip, N.c_u64_p), _ptr(raw_off, N.c_u64_p),
                                               _ptr(cal[0], N.c_float_p) if calibration is not None else None,
                                               _ptr(cal[1], N.c_float_p) if calibration is not None else None,
                                               _ptr(shift, N.c_double_p), _ptr(scale, N.c_double_p), int(window), float(n_sigmas),
                                               int(bool(f32)), seqs, _ptr(seq_off, N.c_u64_p), int(bool(calc_probabilities)),
                                               C.byref(out._c), C.byref(h))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return AsyncBatch(self, h, out, (ptrs, nbytes, samples, read_off, skip, raw_off, shift, scale, seqs, seq_off, cal, ids),
                          wants=self._job_wants(calc_probabilities, raw_off))

    def train_raw_async(self, raw, raw_offsets, shift, scale, seqs: bytes, seq_offsets, window: int = 7,
                        n_sigmas: float = 5.0, f32: bool = True, pooled: bool = False,
                        emissions: bool = True, calibration=None) -> AsyncBatch:
        """dyn_batch_train_raw_async (train.py:163-170: float32 arithmetic, Hampel(7, 5 sigma) by default)."""
        raw, code, shift, scale, cal = self._raw_args(raw, shift, scale, calibration)
        raw_off = np.ascontiguousarray(raw_offsets, dtype=np.uint64)
        seq_off = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = len(raw_off) - 1
        cap = int(self._L.dyn_segment_capacity(self._h, n, _ptr(seq_off, N.c_u64_p)))
        out = TrainBatchResult(n, cap, self.num_kmers, pooled, emissions)
        h = C.c_void_p()
        rc = self._L.dyn_batch_train_raw_async(self._h, n, raw.ctypes.data, code, _ptr(raw_off, N.c_u64_p),
                                               _ptr(cal[0], N.c_float_p) if code & 0xff == 3 else None,
                                               _ptr(cal[1], N.c_float_p) if code & 0xff == 3 else None, _ptr(shift, N.c_double_p), _ptr(scale, N.c_double_p), int(window),
                                               float(n_sigmas), int(bool(f32)), seqs, _ptr(seq_off, N.c_u64_p),
                                               C.byref(out._c), _ptr(out.pooled, N.c_double_p) if pooled else None,
                                               C.byref(h))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return AsyncBatch(self, h, out, (raw, raw_off, shift, scale, seqs, seq_off, cal), wants=JobWants())

    def segment_capacity(self, seq_offsets) -> int:
        """dyn_segment_capacity: rows to allocate for a batch with these sequence offsets."""
        so = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        return int(self._L.dyn_segment_capacity(self._h, len(so) - 1, _ptr(so, N.c_u64_p)))

    def train_async(self, signals, sig_offsets, seqs: bytes, seq_offsets, pooled: bool = False,
                    emissions: bool = True) -> AsyncBatch:
        """dyn_batch_train_async on packed inputs."""
        sig = np.ascontiguousarray(signals, dtype=np.float64)
        sig_off = np.ascontiguousarray(sig_offsets, dtype=np.uint64)
        seq_off = np.ascontiguousarray(seq_offsets, dtype=np.uint64)
        n = len(sig_off) - 1
        cap = int(self._L.dyn_segment_capacity(self._h, n, _ptr(seq_off, N.c_u64_p)))
        out = TrainBatchResult(n, cap, self.num_kmers, pooled, emissions)
        h = C.c_void_p()
        rc = self._L.dyn_batch_train_async(self._h, n, _ptr(sig, N.c_double_p), _ptr(sig_off, N.c_u64_p), seqs,
                                           _ptr(seq_off, N.c_u64_p), C.byref(out._c),
                                           _ptr(out.pooled, N.c_double_p) if pooled else None, C.byref(h))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return AsyncBatch(self, h, out, (sig, sig_off, seqs, seq_off), wants=JobWants())

    def align_batch(self, signals: Sequence, sequences: Sequence[str], calc_probabilities: bool = True,
                    site_ids=None) -> AlignBatchResult:
        with self.batch(signals, sequences, site_ids=site_ids) as b:
            b.align(calc_probabilities)
            res = b.fetch()
        if self._band_retry and calc_probabilities and res.band_margin_low is not None:
            self._retry_bands(res, signals, sequences)
        return res

    def align_batch_guided(self, signals: Sequence, sequences: Sequence[str], guides: Sequence, half_width: int,
                           calc_probabilities: bool = True, refine: int = 1) -> AlignBatchResult:
        """``align_batch`` inside a guided band: ``guides[i]`` is read i's int32 guide, one lattice column per signal sample
        (``dynamont_amd.guide.guide_from_moves`` / ``guide_from_starts`` / ``diagonal_guide``), and every read is aligned in a
        window of ``half_width`` columns on either side of it instead of the band around the fixed diagonal. With
        ``set_band_margin(True)`` the three margin fields are taken against that window. Never retried (``set_band_retry``
        applies to ``align_batch``); not together with ``set_rescale`` / ``set_border_confidence`` (ValueError).
        ``refine`` > 1 (``Batch.set_guide_refine``): up to that many alignments per read, each inside the path the one before
        called, until the guide reproduces itself; the result then carries ``guide_rounds``, ``guide_converged`` (uint32 per
        read) and ``guides`` (every read's guide of its last alignment)."""
        centres = self._guide_centres(signals, guides)
        with self.batch(signals, sequences) as b:
            b.set_guide(centres, half_width)
            if refine != 1:
                b.set_guide_refine(refine)
            b.align(calc_probabilities)
            res = b.fetch()
            if refine != 1:
                res.guide_rounds, res.guide_converged = b.guide_rounds()
                res.guides = b.guide()
            return res

    def align_batch_auto(self, signals: Sequence, sequences: Sequence[str], half_width: int = 32, refine: int = 8,
                         guides: bool = False) -> AlignBatchResult:
        """``align_batch`` inside a guide the library makes itself: the pre-pass of ``Batch.auto_guide(half_width)``, then a
        guided alignment refined up to ``refine`` times (``Batch.set_guide_refine``). No move table, no known starts. The
        result carries ``guide_rounds`` and ``guide_converged`` (uint32 per read) and, with ``guides=True``, ``guides``: every
        read's int32 guide of its last alignment (what ``train_batch_guided`` takes). Restrictions as ``align_batch_guided``."""
        with self.batch(signals, sequences) as b:
            b.auto_guide(half_width)
            if refine != 1:
                b.set_guide_refine(refine)
            b.align(True)
            res = b.fetch()
            res.guide_rounds, res.guide_converged = b.guide_rounds()
            if guides:
                res.guides = b.guide()
            return res

    def train_batch_auto(self, signals: Sequence, sequences: Sequence[str], half_width: int = 32, refine: int = 8,
                         pooled: bool = False) -> TrainBatchResult:
        """``train_batch_guided`` inside self-made guides: ``align_batch_auto`` first, then the Baum-Welch statistics of the
        reads that aligned ok inside their final guides. The result covers those reads only, in input order:
        ``result.reads`` holds their indices into ``signals``, ``result.guide_converged`` the flag of each."""
        al = self.align_batch_auto(signals, sequences, half_width, refine, guides=True)
        keep = [i for i in range(al.n) if al.status[i] == 0]
        tr = self.train_batch_guided([signals[i] for i in keep], [sequences[i] for i in keep], [al.guides[i] for i in keep],
                                     half_width, pooled=pooled)
        tr.reads = np.asarray(keep, dtype=np.int64)
        tr.guide_converged = al.guide_converged[keep] if keep else np.zeros(0, dtype=np.uint32)
        return tr

    @staticmethod
    def _guide_centres(signals: Sequence, guides: Sequence) -> np.ndarray:
        """the batch's guide array: one int32 per signal sample, the reads' guides in batch order"""
        if len(guides) != len(signals):
            raise ValueError("signals and guides differ in length")
        parts = [np.ascontiguousarray(g, dtype=np.int32).ravel() for g in guides]
        for i, (g, s) in enumerate(zip(parts, signals)):
            if g.size != len(s):
                raise ValueError(f"guide {i} holds {g.size} entries for a signal of {len(s)} samples")
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int32)

    def train_batch_guided(self, signals: Sequence, sequences: Sequence[str], guides: Sequence, half_width: int,
                           pooled: bool = False) -> TrainBatchResult:
        """``train_batch`` inside a guided band: the Baum-Welch statistics of every read over the window of
        ``align_batch_guided`` (``half_width`` columns on either side of ``guides[i]``) instead of the band around the fixed
        diagonal. A read whose guide is infeasible fails alone with the training Z-mismatch status."""
        centres = self._guide_centres(signals, guides)
        with self.batch(signals, sequences) as b:
            b.set_guide(centres, half_width)
            b.train_guided()
            return b.fetch_train(pooled)

    def train_batch(self, signals: Sequence, sequences: Sequence[str], pooled: bool = False) -> TrainBatchResult:
        with self.batch(signals, sequences) as b:
            b.train()
            return b.fetch_train(pooled)

    # -- the reference's single-read surface ----------------------------------------------------
    def align(self, signal, sequence: str, calc_probabilities: bool = False) -> dict:
        """aligner_bindings.cpp:132-147,169-176 (single read = batch of one)."""
        return self.align_batch([signal], [sequence], calc_probabilities).read(0)

    def train(self, signal, sequence: str) -> dict:
        """aligner_bindings.cpp:149-163"""
        mean, sd = self.model_table()
        return self.train_batch([signal], [sequence]).read(0, mean, sd)


class RcclComm:
    """dyn_comm_*: the RCCL gather / all-reduce of a one-process-per-GPU job, below Python (no torch needed).
    ``RcclComm.unique_id()`` on rank 0, hand the 128 bytes to the other ranks, then ``RcclComm(id, rank, n_ranks, device)``
    on every rank (collective)."""

    ROW = np.dtype([("signal_pos", "<u4"), ("sequence_pos", "<u4"), ("probability", "<f8")])

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        err = C.create_string_buffer(ERRCAP)
        rc = N.lib().dyn_comm_unique_id(buf, err, ERRCAP)
        if rc != N.DYN_OK:
            _raise(rc, err.value.decode())
        return bytes(buf)

    def __init__(self, unique_id: bytes, rank: int, n_ranks: int, device: int = 0):
        self._L = N.lib()
        self.rank, self.n_ranks = int(rank), int(n_ranks)
        h = C.c_void_p()
        err = C.create_string_buffer(ERRCAP)
        idbuf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        rc = self._L.dyn_comm_create(idbuf, self.rank, self.n_ranks, int(device), C.byref(h), err, ERRCAP)
        if rc != N.DYN_OK:
            _raise(rc, err.value.decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.dyn_comm_destroy(self._h)
            self._h = None

    __del__ = close

    def gather_rows(self, batch, root: int = 0, out=None):
        """(rows, counts): on ``root`` a structured array of every rank's segment rows in rank order; elsewhere rows is
        None. ``batch``: an aligned Batch or an AsyncBatch ticket. Two collectives: the counts (dyn_comm_gather_counts),
        then -- root's buffer allocated for exactly their sum -- the rows. A rank whose batch failed still takes part in
        both (with 0 rows) before its error is raised here, so its peers never block on it. ``out`` (root): a ROW array to
        receive into (e.g. ``pinned_empty(n, RcclComm.ROW)``: the copy off the device is then a plain DMA); one that is too
        small is replaced by a fresh array."""
        counts = np.zeros(self.n_ranks, dtype=np.uint64)
        rc1 = self._L.dyn_comm_gather_counts(self._h, batch._h, _ptr(counts, N.c_u64_p))
        err1 = (self._L.dyn_comm_last_error(self._h) or b"").decode()
        total = int(counts.sum())
        rows = None
        if self.rank == root:
            rows = out if (out is not None and out.dtype == self.ROW and out.size >= max(1, total)) else np.empty(max(1, total), dtype=self.ROW)
        rc = self._L.dyn_comm_gather_rows(self._h, batch._h, int(root), rows.ctypes.data if rows is not None else None,
                                          total if rows is not None else 0, None)
        if rc1 != N.DYN_OK:
            _raise(rc1, err1)
        if rc != N.DYN_OK:
            _raise(rc, (self._L.dyn_comm_last_error(self._h) or b"").decode())
        return (rows[:total] if rows is not None else None), counts

    def _check(self, rc):
        if rc != N.DYN_OK:
            _raise(rc, (self._L.dyn_comm_last_error(self._h) or b"").decode())

    def gather_bytes(self, payload: bytes, root: int = 0):
        """dyn_comm_gather_bytes: one bytes object per rank to ``root`` through the code path of ``gather_rows`` (count
        all-gather, grouped ncclSend / ncclRecv). Returns the list of per-rank payloads on ``root``, None elsewhere."""
        buf = np.frombuffer(payload, dtype=np.uint8) if payload else np.zeros(0, dtype=np.uint8)
        counts = np.zeros(self.n_ranks, dtype=np.uint64)
        self._check(self._L.dyn_comm_gather_bytes(self._h, buf.ctypes.data if buf.size else None, buf.size, int(root), _ptr(counts, N.c_u64_p)))
        if self.rank != root:
            return None
        total = int(counts.sum())
        out = np.empty(max(1, total), dtype=np.uint8)
        self._check(self._L.dyn_comm_gathered_bytes(self._h, out.ctypes.data, total))
        offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        return [out[offs[r]:offs[r + 1]].tobytes() for r in range(self.n_ranks)]

    def allreduce(self, x: np.ndarray, op: str = "sum") -> np.ndarray:
        """dyn_comm_allreduce_f64: elementwise sum / max over the ranks of a float64 vector (a copy is returned)."""
        out = np.ascontiguousarray(x, dtype=np.float64).copy()
        self._check(self._L.dyn_comm_allreduce_f64(self._h, _ptr(out, N.c_double_p), out.size, {"sum": 0, "max": 1}[op]))
        return out

    def allreduce_pooled(self, batch, num_kmers: int) -> np.ndarray:
        out = np.empty(3 * int(num_kmers))
        rc = self._L.dyn_comm_allreduce_pooled(self._h, batch._h, _ptr(out, N.c_double_p))
        if rc != N.DYN_OK:
            _raise(rc, (self._L.dyn_comm_last_error(self._h) or b"").decode())
        return out


class MultiAligner:
    """dyn_multi_*: one handle driving several GPUs of a node from ONE process. Reads of a batch are cut into
    contiguous ranges of equal lattice work, one per device; results come back in the layout of a single-device
    batch. ``devices``: HIP ordinals (an ordinal may repeat, e.g. ``[0, 0]`` = two pipelines on one GPU)."""

    def __init__(self, model_file: str, pore, devices: Sequence[int], mode: str = "basic", threads: int = 1, band: int = 400):
        if isinstance(pore, str):
            pore = pore_type(pore)
        self._L = N.lib()
        ids = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        err = C.create_string_buffer(ERRCAP)
        rc = self._L.dyn_multi_create(str(model_file).encode(), int(pore), str(mode).encode(), int(threads), int(band), ids,
                                      len(devices), C.byref(h), err, ERRCAP)
        if rc != N.DYN_OK:
            _raise(rc, err.value.decode())
        self._h = h
        info = N.DynInfo()
        self._L.dyn_aligner_info(self._L.dyn_multi_handle(h, 0), C.byref(info))
        self.kmer_size, self.num_kmers, self.n_devices = int(info.kmer_size), int(info.num_kmers), len(devices)

    def close(self):
        if getattr(self, "_h", None):
            self._L.dyn_multi_destroy(self._h)
            self._h = None

    __del__ = close

    def last_error(self) -> str:
        return (self._L.dyn_multi_last_error(self._h) or b"").decode(errors="replace")

    def set_site_summary(self, num_sites: int, capacity: int | None = None) -> None:
        """Not supported, dense or sparse (``capacity=``): the per-site table lives on ONE device's handle and the reads of a
        batch are cut over the devices. Use one ``Aligner`` per device and add the tables (they are integers)."""
        raise NotImplementedError("MultiAligner has no per-site summary (Aligner.set_site_summary): use one Aligner per device "
                                  "and add their tables")

    def set_site_histogram(self, bins: int, lo: float = 0.0, hi: float = 0.0) -> None:
        """Not supported, as ``set_site_summary`` is not: the histograms live beside ONE device's table. Use one ``Aligner`` per
        device and add the counters (they are integers)."""
        raise NotImplementedError("MultiAligner has no per-site histograms (Aligner.set_site_histogram): use one Aligner per device "
                                  "and add their tables")

    def set_site_model(self, lo: int, m: dict, accept=(0, 2)) -> dict:
        """Not supported, as ``set_site_summary`` is not: the model lives beside ONE device's table."""
        raise NotImplementedError("MultiAligner has no per-site model (Aligner.set_site_model): use one Aligner per device")

    def set_site_calls(self, on: bool) -> None:
        """Not supported, as ``set_site_summary`` is not."""
        raise NotImplementedError("MultiAligner has no per-read site calls (Aligner.set_site_calls): use one Aligner per device")

    def site_summary_add(self, lo: int, summary: dict, histogram: dict | None = None) -> None:
        """Not supported, as ``set_site_summary`` is not."""
        raise NotImplementedError("MultiAligner has no per-site summary (Aligner.site_summary_add): use one Aligner per device "
                                  "and add their tables")

    def site_table_pack(self, lo: int = 0, hi: int | None = None) -> dict:
        """Not supported, as ``set_site_summary`` is not: pack the table of each device's ``Aligner``."""
        raise NotImplementedError("MultiAligner has no per-site summary (Aligner.site_table_pack): use one Aligner per device "
                                  "and merge their packed tables (Aligner.site_summary_merge)")

    def site_summary_merge(self, packed: dict, offset: int = 0) -> None:
        """Not supported, as ``set_site_summary`` is not."""
        raise NotImplementedError("MultiAligner has no per-site summary (Aligner.site_summary_merge): use one Aligner per device "
                                  "and merge their packed tables")

    def site_compare(self, lo: int = 0, hi: int | None = None, other_lo: int | None = None) -> dict:
        """Not supported, as ``set_site_histogram`` is not."""
        raise NotImplementedError("MultiAligner has no per-site histograms (Aligner.site_compare): use one Aligner per device "
                                  "and add their tables")

    def site_mixture(self, lo: int = 0, hi: int | None = None, other_lo: int | None = None, max_iters: int = 128, tol: float = 1e-3,
                     min_n: int = 8) -> dict:
        """Not supported, as ``set_site_histogram`` is not."""
        raise NotImplementedError("MultiAligner has no per-site histograms (Aligner.site_mixture): use one Aligner per device "
                                  "and add their tables")

    def _cap(self, seq_off) -> int:
        return int(self._L.dyn_segment_capacity(self._L.dyn_multi_handle(self._h, 0), len(seq_off) - 1, _ptr(seq_off, N.c_u64_p)))

    def align_batch(self, signals: Sequence, sequences: Sequence[str], calc_probabilities: bool = True) -> AlignBatchResult:
        sig, sig_off, seqs, seq_off = _pack(signals, sequences)
        out = AlignBatchResult(len(sequences), self._cap(seq_off))
        rc = self._L.dyn_multi_align_batch(self._h, out.n, _ptr(sig, N.c_double_p), _ptr(sig_off, N.c_u64_p), seqs,
                                           _ptr(seq_off, N.c_u64_p), int(bool(calc_probabilities)), C.byref(out._c))
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return out

    def train_batch(self, signals: Sequence, sequences: Sequence[str], pooled: bool = False) -> TrainBatchResult:
        sig, sig_off, seqs, seq_off = _pack(signals, sequences)
        out = TrainBatchResult(len(sequences), self._cap(seq_off), self.num_kmers, pooled)
        rc = self._L.dyn_multi_train_batch(self._h, out.n, _ptr(sig, N.c_double_p), _ptr(sig_off, N.c_u64_p), seqs,
                                           _ptr(seq_off, N.c_u64_p), C.byref(out._c),
                                           _ptr(out.pooled, N.c_double_p) if pooled else None)
        if rc != N.DYN_OK:
            _raise(rc, self.last_error())
        return out
