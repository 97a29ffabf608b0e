#!/usr/bin/env python
"""``dynamont-train`` counterpart (reference: src/dynamont/segmentation/train.py).

Batch Baum-Welch driver: per batch of reads one ``train_batch`` on the GPU, then a parameter
update, a model file ``trained_{epoch}_{batch}.model``, a ``params.csv`` row and a re-evaluation
of Z with the new model (train.py:178-249).

Aggregation (``--aggregate``):
  window-mean  the reference's estimator: every parameter becomes the mean of a 100-deep sliding
               window of PER-READ estimates (ManagedList, train.py:19-46,106,213,220);
  pooled       one M-step from the batch-pooled sufficient statistics (w, s1, s2) -- the quantity
               BASELINE.json config 5 all-reduces across GPUs (dynamont_amd.parallel).

Deliberate differences from the reference (not silently "fixed"):
  * k-mer <-> parameter pairing is by k-mer code; the reference zips file order with code order
    (utils.py:171-175), which mislabels RNA models;
  * as in the reference, updated TRANSITIONS are logged but never reach the native aligner
    (no setter exists, aligner_bindings.cpp:191-216): every read trains with the pore defaults.

``--guide-moves HW`` (build-only, default 0 = off): every read is trained, and its Z re-evaluated, inside a window of HW
lattice columns around the guide its basecaller move table (``mv:B:c``) gives (``Aligner.train_batch_guided``, INTEGRATION.md
section 3) instead of the band around the fixed diagonal; a read without a usable move table is skipped and counted.

``--guide-auto HW [--guide-rounds R]`` (build-only, default 0 = off; not together with ``--guide-moves``): the same guided
training path with a guide the library makes itself -- ``Batch.auto_guide(HW)``, refined up to R alignments
(``Batch.set_guide_refine``) -- so that no ``mv`` tag is needed. A read that does not align inside its own guide is reported
and left out of its batch; the reads whose guide did not reproduce itself within R alignments are trained and counted.
"""
from __future__ import annotations

import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser, Namespace
from collections import deque
from datetime import datetime
from os import makedirs
from os.path import basename, dirname, exists, join

import numpy as np

from dynamont_amd import Aligner, __version__
from dynamont_amd import guide as guide_mod
from dynamont_amd.pod5_io import get_signal, iter_basecalls, open_pod5
from dynamont_amd.segmentation.utils import (cnt_nts_ratios, get_model, hampel, kmer_of_code, read_kmer_model,
                                             write_kmer_model, write_kmer_model_arrays)

WINDOW = 100


class ManagedList:
    """Bounded list of recent values (train.py:19-46)."""

    def __init__(self, values, max_size=WINDOW):
        self.values = deque(values, maxlen=max_size)

    def add(self, value):
        self.values.append(value)

    def get_list(self):
        return list(self.values)

    def __repr__(self):
        return f"ManagedList({list(self.values)})"

    def mean(self):
        return None if len(self.values) == 0 else np.mean(self.values)

    def median(self):
        return None if len(self.values) == 0 else np.median(self.values)


class ManagedTable:
    """ManagedList for every k-mer at once: a ring of dense (mean, stdev) vectors. ``add`` appends
    one per-read estimate for EVERY k-mer (the reference appends the full dense model of each
    read, train.py:202-205); ``mean`` is the column mean over the filled part of the window."""

    def __init__(self, mean0: np.ndarray, sd0: np.ndarray, max_size=WINDOW):
        self.buf = np.empty((max_size, 2, mean0.size))
        self.buf[0, 0] = mean0
        self.buf[0, 1] = sd0
        self.count = 1
        self.head = 1
        self.max_size = max_size

    def add(self, mean: np.ndarray, sd: np.ndarray):
        self.buf[self.head % self.max_size, 0] = mean
        self.buf[self.head % self.max_size, 1] = sd
        self.head += 1
        self.count = min(self.count + 1, self.max_size)

    def mean(self):
        m = self.buf[:self.count].mean(axis=0)
        return m[0], m[1]


def parse(argv=None) -> Namespace:
    """Flags of train.py:48-66 plus the build-only ones."""
    p = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, prog="dynamont-train")
    p.add_argument("-r", "--raw", type=str, required=True, metavar="PATH", help="Path to raw ONT data. [POD5|FAST5]")
    p.add_argument("-b", "--basecalls", type=str, required=True, metavar="BAM", help="Basecalls of ONT training data as .bam file")
    p.add_argument("-o", "--outdir", type=str, required=True, metavar="PATH", help="Outpath to write files")
    p.add_argument("-p", "--pore", type=str, required=True, choices=["rna002", "rna004", "dna_r10_260bps", "dna_r10_400bps"], help="Pore generation used to sequence the data")
    p.add_argument("--model_path", type=str, help="Which initial kmer models to use for training")
    p.add_argument("--batch_size", type=int, default=24, help="Number of reads to train before updating")
    p.add_argument("--max_batches", type=int, default=None, help="Numbers of batches to train each epoch")
    p.add_argument("-e", "--epochs", type=int, default=1, help="Number of training epochs")
    p.add_argument("-q", "--qscore", type=float, default=10.0, help="Minimal allowed quality score")
    p.add_argument("--version", action="version", version=f"%(prog)s {__version__}")
    p.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    p.add_argument("--aggregate", choices=["window-mean", "pooled"], default="window-mean",
                   help="parameter update: the reference's sliding-window mean of per-read estimates, or a pooled M-step")
    p.add_argument("--no-timestamp", action="store_true", help="write into OUTDIR itself (the reference appends a timestamp)")
    p.add_argument("--host-preprocess", action="store_true", help="normalise + Hampel-filter with NumPy on the host instead of on the GPU (same values)")
    p.add_argument("--reference-zcheck", action="store_true",
                   help="also refuse the reads the reference's |Zf - Zb| / size > 1e-8 rule refuses (NT_aligner_api.cpp:619-625): "
                        "one more Z-only forward sweep per read; default: the posterior chain's own mass check")
    p.add_argument("--guide-moves", type=int, default=0, metavar="HW",
                   help="train inside a window of HW lattice columns on either side of the guide the basecaller's move table "
                        "(mv:B:c) gives, instead of the band around the diagonal; reads without a move table are skipped (0: off)")
    p.add_argument("--guide-auto", type=int, default=0, metavar="HW",
                   help="train inside a window of HW lattice columns on either side of a guide made on the GPU from the signal and "
                        "the sequence alone (no move table needed); not together with --guide-moves (0: off)")
    p.add_argument("--guide-rounds", type=int, default=8, metavar="R",
                   help="with --guide-auto: alignments per read at the most while its guide is refined (1 .. 64)")
    args = p.parse_args(argv)
    if args.guide_auto and args.guide_moves:
        p.error("--guide-auto and --guide-moves are mutually exclusive")
    return args


def _code_order(model: dict, k: int, rna: bool):
    n = 4 ** k
    names = [kmer_of_code(c, k, rna) for c in range(n)]
    mean = np.array([model[s][0] for s in names])
    sd = np.array([model[s][1] for s in names])
    return names, mean, sd


def _move_guide(rec, n_samples: int, n_bases: int, k: int):
    """the read's guide from its ``mv`` tag, or None: no tag, no move in the table, or a sequence shorter than a k-mer. The
    signal starts at sp + ts, where the move table begins (ts = 0 for guide_from_moves); the sequence is the aligner's (RNA:
    reversed into signal order and padded, so reverse=False -- INTEGRATION.md section 3's orientation rule)."""
    if not rec.has_tag("mv"):
        return None
    try:
        return guide_mod.guide_from_moves(rec.get_tag("mv"), n_samples, n_bases, k, ts=0, reverse=False)
    except ValueError:
        return None


def read_items(data_path, basecalls, pore, minq, raw: bool = False, guide_moves: int = 0, k: int = 0):
    """Read filters + preprocessing of train.py:125-176, one item per accepted read:
    (signal, sequence, readid). With ``raw=True`` the arithmetic is left to the device and the item
    is ((raw float32 slice, shift, scale), sequence, readid) for ``Aligner.batch_raw(..., window=7,
    n_sigmas=5.0, f32=True)``. With ``guide_moves`` > 0 (``k``: the model's k-mer size) an item carries a fourth entry, the
    read's int32 guide from its move table (one lattice column per sample of the cut signal), and a read without a usable
    table yields "noguide"."""
    old_file, r5 = None, None
    for rec in iter_basecalls(basecalls):
        if minq and rec.get_tag("qs") < minq:
            yield "qskip"
            continue
        seq = rec.query_sequence
        counts = cnt_nts_ratios(seq)
        if any(counts[b] >= 0.6 for b in counts):  # homopolymer-like artefacts (train.py:136-142)
            continue
        readid = rec.get_tag("pi") if rec.has_tag("pi") else rec.query_name
        sp = rec.get_tag("sp") if rec.has_tag("sp") else 0
        start, end = sp + rec.get_tag("ts"), sp + rec.get_tag("ns")
        shift, scale = rec.get_tag("sm"), rec.get_tag("sd")
        ont_file = join(data_path, rec.get_tag("fn"))
        if old_file != ont_file:
            old_file, r5 = ont_file, open_pod5(ont_file)
        try:
            signal = get_signal(r5, readid, calibrated=shift <= 400)[start:end]
        except Exception:  # noqa: BLE001
            yield "mismatch"
            continue
        signal = np.array(signal, dtype=np.float32 if signal.dtype.kind != "f" else signal.dtype, copy=True)
        if "rna" in pore:
            seq = seq[::-1]
            if not seq.startswith("AAAAAAAAA"):
                seq = "AAAAAAAAA" + seq
        extra = ()
        if guide_moves > 0:  # after the reversal and the pad: the guide is over the aligner's own sequence
            g = _move_guide(rec, len(signal), len(seq), k)
            if g is None:
                yield "noguide"
                continue
            extra = (g,)
        if raw:
            yield ((signal, float(shift), float(scale)), seq, readid) + extra
            continue
        signal -= shift   # float32 arithmetic when the reader returns float32, as in train.py:168-169
        signal /= scale
        hampel(signal, 7, 5.0)
        yield (signal, seq, readid) + extra


def _train_items(al: Aligner, items, pooled: bool, raw: bool, guide_moves: int = 0):
    """guide_moves > 0: the items carry their guides (read_items) and the batch trains inside them"""
    if not raw:
        if guide_moves > 0:
            return al.train_batch_guided([x[0] for x in items], [x[1] for x in items], [x[3] for x in items], guide_moves, pooled=pooled)
        return al.train_batch([x[0] for x in items], [x[1] for x in items], pooled=pooled)
    f32 = items[0][0][0].dtype == np.float32
    with al.batch_raw([x[0][0] for x in items], [x[1] for x in items], [x[0][1] for x in items],
                      [x[0][2] for x in items], window=7, n_sigmas=5.0, f32=f32) as b:
        if guide_moves > 0:
            b.set_guide(np.concatenate([x[3] for x in items]), guide_moves)
            b.train_guided()
        else:
            b.train()
        return b.fetch_train(pooled)


def _attach_auto_guides(al: Aligner, items, raw: bool, half_width: int, rounds: int):
    """--guide-auto: one refined, self-guided alignment of the batch (Batch.auto_guide, Batch.set_guide_refine). Returns the items
    that aligned ok, each with its final guide as fourth entry (what the guided training path takes), the (readid, error) pairs
    of the others and the number of kept reads whose guide did not converge."""
    if raw:
        f32 = items[0][0][0].dtype == np.float32
        b = al.batch_raw([x[0][0] for x in items], [x[1] for x in items], [x[0][1] for x in items], [x[0][2] for x in items],
                         window=7, n_sigmas=5.0, f32=f32)
    else:
        b = al.batch([x[0] for x in items], [x[1] for x in items])
    with b:
        b.auto_guide(half_width)
        if rounds != 1:
            b.set_guide_refine(rounds)
        b.align(True)
        res = b.fetch()
        _, converged = b.guide_rounds()
        guides = b.guide()
    kept = [tuple(x[:3]) + (guides[j],) for j, x in enumerate(items) if res.status[j] == 0]
    failed = [(x[2], res.error(j)) for j, x in enumerate(items) if res.status[j] != 0]
    return kept, failed, int(sum(1 for j in range(len(items)) if res.status[j] == 0 and not converged[j]))


def _z_items(al: Aligner, items, raw: bool, guide_moves: int = 0):
    """guide_moves > 0: the guided Z-only job over the same guides, so that the Z change compares like with like"""
    if not raw:
        if guide_moves > 0:
            return al.align_batch_guided([x[0] for x in items], [x[1] for x in items], [x[3] for x in items], guide_moves,
                                         calc_probabilities=False)
        return al.align_batch([x[0] for x in items], [x[1] for x in items], calc_probabilities=False)
    f32 = items[0][0][0].dtype == np.float32
    with al.batch_raw([x[0][0] for x in items], [x[1] for x in items], [x[0][1] for x in items],
                      [x[0][2] for x in items], window=7, n_sigmas=5.0, f32=f32) as b:
        if guide_moves > 0:
            b.set_guide(np.concatenate([x[3] for x in items]), guide_moves)
        b.align(False)
        return b.fetch()


def train(data_path: str, basecalls: str, batch_size: int, epochs: int, param_file: str, mode: str, model_path: str,
          max_batches, pore: str, minq=None, device: int = 0, aggregate: str = "window-mean", comm=None,
          host_preprocess: bool = False, reference_zcheck: bool = False, guide_moves: int = 0, guide_auto: int = 0,
          guide_rounds: int = 8) -> None:
    """Counterpart of train.py:68-253. ``comm`` (optional, dynamont_amd.parallel.Comm): multi-GPU
    run -- accepted reads are dealt round-robin to the ranks (each rank fills ``batch_size`` reads of
    its own per batch, so all ranks reach a batch boundary on the same read), the pooled sufficient
    statistics, transition counts and Z changes are summed over ranks, every rank computes the same
    model, and rank 0 owns params.csv and the model files in ``outdir``. ``guide_moves`` > 0: the guided band around every
    read's move-table guide at that half width (the guide travels with its item, so a rank trains the reads it is dealt with
    their own guides; run with one rank so far). ``guide_auto`` > 0: the same path with guides the library makes itself at
    that half width, refined up to ``guide_rounds`` alignments (no move table needed)."""
    if guide_moves < 0:
        raise ValueError("--guide-moves must be >= 0")
    if guide_auto < 0 or (guide_auto and guide_moves):
        raise ValueError("--guide-auto must be >= 0 and is not combined with --guide-moves")
    guide_hw = guide_moves or guide_auto  # the half width of the guided training path, whichever made the guides
    if mode != "basic":
        print(f"Mode {mode} not implemented", file=sys.stderr)
        sys.exit(1)
    rank, world = (comm.rank, comm.world) if comm is not None else (0, 1)
    if world > 1 and aggregate != "pooled":
        raise ValueError("multi-GPU training needs --aggregate pooled (per-read windows are rank-local)")
    model = read_kmer_model(model_path)
    outdir = dirname(param_file)
    if rank != 0:  # private copies of the per-batch model files; params.csv is rank 0's
        outdir = join(outdir, f".rank{rank}")
        makedirs(outdir, exist_ok=True)
        param_file = join(outdir, "params.csv")
    trained_model = join(outdir, "trained_0_0.model")
    write_kmer_model(trained_model, model)
    transition_params = {"e1": 1.0, "m1": 0.03, "e2": 0.97}  # train.py:76-82 (logged only)
    probe = Aligner(trained_model, pore, device="host")
    k, rna, K = probe.kmer_size, probe.rna, probe.num_kmers
    names, mean0, sd0 = _code_order(model, k, rna)
    # the model file keeps the row order of the file it started from: row -> k-mer code, once
    code_of_name = {name: c for c, name in enumerate(names)}
    code_of_row = np.fromiter((code_of_name[name] for name in model), dtype=np.int64, count=len(model))
    file_kmers = "".join(model).encode()
    table = ManagedTable(mean0, sd0)
    trans = {p: ManagedList([v]) for p, v in transition_params.items()}
    any_seen = False
    al = None
    i = qskips = mismatches = noguides = auto_failed = auto_open = 0
    with open(param_file, "w") as pw:
        pw.write("epoch,batch,read," + "".join(p + "," for p in transition_params) + "Zchange\n")
        for e in range(epochs):
            items, cbatch, accepted = [], 0, 0
            for it in read_items(data_path, basecalls, pore, minq, raw=not host_preprocess, guide_moves=guide_moves, k=k):
                if it == "noguide":
                    noguides += 1
                    continue
                if it == "qskip":
                    qskips += 1
                    continue
                if it == "mismatch":
                    mismatches += 1
                    continue
                accepted += 1
                if (accepted - 1) % world == rank:
                    items.append(it)
                if accepted % (batch_size * world):  # a batch = batch_size reads on EVERY rank
                    continue
                print("============================", file=sys.stderr)
                print(f"{datetime.now().strftime('%Y-%m-%d_%H-%M-%S')}: Training epoch: {e}, reads: {i}, batch: {cbatch}\n{transition_params}", file=sys.stderr)
                cbatch += 1
                # train.py:179 builds an Aligner from the model file of the previous batch; the one kept here holds exactly
                # those values (set_model below; a float64 survives the file's shortest decimal representation unchanged)
                if al is None:
                    al = Aligner(trained_model, pore, mode="basic", threads=4, band=400, device=device)
                    al.set_train_zcheck(reference_zcheck)
                cur_mean, cur_sd = al.model_table()
                if guide_auto > 0:
                    items, failed, not_converged = _attach_auto_guides(al, items, not host_preprocess, guide_auto, guide_rounds)
                    auto_failed += len(failed)
                    auto_open += not_converged
                    for readid, err in failed:
                        print(f"error: native, {err} Sid: {readid} (no alignment inside its own guide: left out)", file=sys.stderr)
                    if not items:
                        continue
                res = _train_items(al, items, aggregate == "pooled", raw=not host_preprocess, guide_moves=guide_hw)
                preZ = {}
                for j, readid in enumerate(x[2] for x in items):
                    if res.status[j] != 0:
                        print(f"error: native, {res.error(j)} T: {len(items[j][0][0] if not host_preprocess else items[j][0])} N: {len(items[j][1])} Sid: {readid}", file=sys.stderr)
                        print(f"No segmentation calculated for {readid} in {e}: {trained_model}.", file=sys.stderr)
                        continue
                    i += 1
                    preZ[j] = float(res.Z[j])
                    t = res.transitions[3 * j:3 * j + 3]
                    trans["m1"].add(float(t[0]))
                    trans["e1"].add(float(t[1]))
                    trans["e2"].add(float(t[2]))
                    code, m, s = res.sparse(j)
                    # the read's dense model: the current one with the touched k-mers replaced (train.py:190-197); only the
                    # window mean needs all of it, the "weird training" test below needs k-mer 0
                    at0 = np.nonzero(code == 0)[0]
                    mean0_read = float(m[at0[0]]) if len(at0) else float(cur_mean[0])
                    if mean0_read < 0.5:  # "skip weird trainings": polyA k-mer mean collapsed (train.py:198-199)
                        continue
                    any_seen = True
                    if aggregate == "window-mean":
                        dm, ds = cur_mean.copy(), cur_sd.copy()
                        dm[code] = m
                        ds[code] = s
                        table.add(dm, ds)
                print(f"Zs: {list(preZ.values())}", file=sys.stderr)
                if comm is not None:  # reads trained so far and pooled transition estimate over all ranks
                    ok = [j for j in preZ]
                    tot = comm.allreduce_sum(np.array([len(ok), res.trans_counts[0::2][ok].sum(), res.trans_counts[1::2][ok].sum()]))
                    i_global = getattr(train, "_i_global", 0) + int(tot[0])
                    train._i_global = i_global
                    m1 = tot[1] / (tot[1] + tot[2]) if tot[1] + tot[2] > 0 else 0.0
                    pooled_trans = {"e1": 1.0, "m1": m1, "e2": 1.0 - m1 if tot[1] + tot[2] > 0 else 0.0}
                pw.write(f"{e},{cbatch},{i if comm is None else i_global},")
                for p in transition_params:
                    transition_params[p] = trans[p].mean() if comm is None else pooled_trans[p]
                    pw.write(f"{transition_params[p]},")
                if aggregate == "pooled":
                    pooled = res.pooled
                    if comm is not None:
                        pooled = comm.allreduce_sum(pooled)
                    w, s1, s2 = pooled[:K], pooled[K:2 * K], pooled[2 * K:]
                    hit = w > 0
                    new_mean, new_sd = cur_mean.copy(), cur_sd.copy()
                    new_mean[hit] = s1[hit] / w[hit]
                    var = np.maximum(s2[hit] / w[hit] - new_mean[hit] ** 2, 1e-12)  # NT_aligner_api.cpp:523-529
                    new_sd[hit] = np.sqrt(var)
                elif any_seen:
                    new_mean, new_sd = table.mean()
                else:
                    new_mean, new_sd = cur_mean, cur_sd
                trained_model = join(outdir, f"trained_{e}_{cbatch}.model")
                # write_kmer_model(trained_model, {name: [new_mean[c], new_sd[c]] ...}) (train.py:221-224), same bytes
                write_kmer_model_arrays(trained_model, file_kmers, k, np.asarray(new_mean)[code_of_row], np.asarray(new_sd)[code_of_row])
                pw.flush()
                # rerun with the new model to compare Zs (train.py:226-242)
                al.set_model(new_mean, new_sd)  # = Aligner(trained_model, ...) of train.py:227
                post = _z_items(al, items, raw=not host_preprocess, guide_moves=guide_hw)
                dZ = np.array([float(post.Z[j]) - z for j, z in preZ.items() if post.status[j] == 0])
                print(f"Z changes: {dZ}", file=sys.stderr)
                if comm is not None:
                    sz = comm.allreduce_sum(np.array([dZ.sum(), float(len(dZ))]))
                    deltaZ = sz[0] / sz[1] if sz[1] else 0.0
                else:
                    deltaZ = np.mean(dZ) if len(dZ) else 0.0
                pw.write(f"{deltaZ}\n")
                pw.flush()
                items = []
                if max_batches is not None and cbatch >= max_batches:
                    break
    train._i_global = 0
    print("Done training", file=sys.stderr)
    print(f"Skipped reads due to low quality: {qskips}", file=sys.stderr)
    if guide_moves > 0:
        print(f"Skipped reads due to a signal mismatch: {mismatches}", file=sys.stderr)
        print(f"Skipped reads without a move table (mv): {noguides}", file=sys.stderr)
    if guide_auto > 0:
        print(f"Skipped reads due to a signal mismatch: {mismatches}", file=sys.stderr)
        print(f"Reads left out (no alignment inside their own guide): {auto_failed}", file=sys.stderr)
        print(f"Reads whose guide did not converge within {guide_rounds} alignments: {auto_open}", file=sys.stderr)


def main(argv=None) -> None:
    args = parse(argv)
    # under torch.distributed.run: every rank trains its own shard of each batch on its own GPU and the
    # pooled sufficient statistics are summed over ranks (BASELINE.json config 5)
    from dynamont_amd import parallel
    comm, local_rank = parallel.init_from_env()
    outdir = args.outdir if args.no_timestamp else args.outdir + f'_{datetime.now().strftime("%Y-%m-%d_%H-%M-%S")}'
    if comm is not None:
        outdir = parallel.broadcast_str(comm, outdir)  # one time stamp for the whole job
    makedirs(outdir, exist_ok=True)  # every rank gets here; the first one wins
    param_file = join(outdir, "params.csv")
    if args.model_path:
        model_path = args.model_path
        assert exists(model_path), "Model path does not exist"
    else:
        model_path = get_model(args.pore)
        assert exists(model_path), f"Default model not found for pore: {args.pore}, {model_path}"
    print(f"Loaded model: {basename(model_path)}", file=sys.stderr)
    if comm is not None and comm.rank == 0:
        print(f"exchange: {comm.implementation}", file=sys.stderr, flush=True)
    # a failing rank ends the whole job instead of leaving the others in their next all-reduce (parallel.abort)
    with parallel.abort_on_error(comm):
        train(args.raw, args.basecalls, args.batch_size, args.epochs, param_file, "basic", model_path, args.max_batches,
              args.pore, args.qscore, device=local_rank if comm else args.device, aggregate=args.aggregate, comm=comm,
              host_preprocess=args.host_preprocess, reference_zcheck=args.reference_zcheck, guide_moves=args.guide_moves,
              guide_auto=args.guide_auto, guide_rounds=args.guide_rounds)
        if comm is not None:
            comm.close()  # (collective: every rank has finished its exchanges)


if __name__ == "__main__":
    main()
