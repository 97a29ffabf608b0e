#!/usr/bin/env python
"""``dynamont-resquiggle`` counterpart (reference: src/dynamont/segmentation/segment.py).

Same command line, same CSV bytes, same ``.errors`` lines. The reference forks one worker per
CPU core, each aligning one read at a time; here one process drives one MI355X and hands the
aligner batches of reads (``--batch-reads``), while a writer thread streams the zstd CSV.

  P1 preprocessing   segment.py:141-158  -> prepare_job()
  P3 job generator   segment.py:189-258  -> generate_jobs()
  P4 writer          segment.py:69-107   -> listener()
"""
from __future__ import annotations

import os
import queue as queue_mod
import sys
import threading
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser, Namespace
from collections import OrderedDict
from os import makedirs
from os.path import basename, dirname, exists, isdir, join, splitext

import numpy as np

from dynamont_amd import Aligner, __version__
from dynamont_amd.pod5_io import VbzSlice, get_signal, get_signal_adc, get_signal_chunks, iter_basecalls, open_pod5
from dynamont_amd.segmentation.utils import get_model, hampel, segmentation_to_string
from dynamont_amd.zstd_io import open_writer


def _stamp(name: str) -> None:
    """DYN_CLI_TRACE=1: a timeline of the run on stderr, seconds since the process was started (DYN_CLI_T0 = the parent's
    time.time() at Popen, else since this module was imported) -- where a cold start goes (tools/cold_start_trace.py)"""
    import os
    import time
    if os.environ.get("DYN_CLI_TRACE"):
        t0 = float(os.environ.get("DYN_CLI_T0") or _IMPORTED_AT)
        print("[cli %8.3f s] %s" % (time.time() - t0, name), file=sys.stderr, flush=True)


import time as _time  # noqa: E402

_IMPORTED_AT = _time.time()

CSV_HEADER = b"readid,signalid,start,end,basepos,base,motif,state,posterior_probability,polish\n"
# --event-stats: every row also carries the per-segment signal levels (Aligner.set_event_stats)
CSV_HEADER_EVENTS = CSV_HEADER[:-1] + b",level_mean,level_stdv,level_median\n"
# --segment-scores W: ... and, after those, the per-border segment scores (Aligner.set_segment_scores)
CSV_COLUMNS_SCORES = b",median_delta,mad_delta,homogeneity"
# --border-confidence W: ... and, after those, the per-border posterior confidence (Aligner.set_border_confidence)
CSV_COLUMNS_BORDERS = b",border_probability,border_window_probability"
# --posterior-samples K: ... and, after those, one field with the K sampled starts of the segment (Aligner.set_posterior_samples)
CSV_COLUMNS_SAMPLES = b",sample_starts"
# --border-interval MASS: ... and, after those, the credible interval and spread of the segment's start (Aligner.set_border_interval)
CSV_COLUMNS_INTERVALS = b",border_lo,border_hi,border_mean,border_sd"
# --soft-levels: ... and, after those, the posterior-weighted dwell, level and spread of the base (Aligner.set_soft_levels)
CSV_COLUMNS_SOFT = b",soft_dwell,soft_mean,soft_stdv"
POLYA = "AAAAAAAAA"

MAX_SAMPLES_IN_FLIGHT = 512 << 20  # ~1 GB of pinned int16 staging + ~4 GB of float64 on the device, whatever --depth says
LAST_RUN: dict = {}  # what the native sink of the last single-process run reported at close (bench.py's e2e_cli record)
RAW_CACHE: OrderedDict | None = None
RAW_CACHE_SIZE = 32  # open readers kept (the reference keeps 3, segment.py:44,123-139: "the pod5 files should more or less be
                     # ordered"); a basecall file over a directory of pod5 files interleaves them, a batch of 1 024 reads then touches
                     # many, and re-opening one costs its index -- a memory-mapped reader that is merely kept costs nothing
ZSTD_WORKERS = 0    # compression threads of the writer (0: up to 8 host cores; level 3 as the reference)
ZSTD_PARALLEL_FRAMES = False  # --parallel-zstd-frames: consecutive independent frames instead of the reference's one


def parse(argv=None) -> Namespace:
    """Flags of segment.py:47-67 plus the build-only GPU flags."""
    p = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, prog="dynamont-resquiggle")
    p.add_argument("-r", "--raw", type=str, required=True, metavar="PATH", help="Path to raw ONT data. [POD5]")
    p.add_argument("-b", "--basecalls", type=str, required=True, metavar="BAM", help="Basecalls of ONT training data as .bam file")
    p.add_argument("-o", "--outfile", type=str, required=True, help="Path to output file. Will be zstd level 3 compressed. If directory is given, will write to dynamont.csv in that directory.")
    p.add_argument("--mode", type=str, required=True, choices=["basic", "resquiggle"], help="Segmentation algorithm used for segmentation")
    p.add_argument("--processes", type=int, default=1, help="Kept for command-line compatibility; the GPU build runs one process per device")
    p.add_argument("-p", "--pore", type=str, required=True, choices=["rna002", "rna004", "dna_r10_260bps", "dna_r10_400bps"], help="Pore generation used to sequence the data")
    p.add_argument("--model_path", type=str, help="Which kmer model to use for segmentation")
    p.add_argument("-q", "--qscore", type=float, default=0.0, help="Minimal allowed quality score")
    p.add_argument("--version", action="version", version=f"%(prog)s {__version__}")
    # build-only
    p.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    p.add_argument("--batch-reads", type=int, default=1024, help="Reads per GPU batch")
    p.add_argument("--mem-budget", type=float, default=0.0, help="HBM budget for lattice workspaces in GiB (0 = 90%% of free)")
    p.add_argument("--depth", type=int, default=12, help="batches in flight at once, from submission to the written rows "
                   "(batches that wait while the GPU is busy are merged into one launch, whose queue balances reads of unequal "
                   "length: with 12 in flight launches of 3 batches follow each other)")
    p.add_argument("--zstd-level", type=int, default=3, help="compression level of the output frame (3: the reference's, "
                   "segment.py:60,74; on these rows level 1 is 1.8x faster AND 6 %% smaller)")
    p.add_argument("--host-threads", type=int, default=0, help="threads that compress the output (0: the CPUs this process "
                   "may use minus 4, at most 16 -- zstd level 3 of 230 MB of rows per 1 024-read batch is the largest host cost)")
    p.add_argument("--strict-ties", type=str, default="ties", choices=["off", "ties", "start", "all"],
                   help="reproduce the reference's sums bit for bit (dyn_aligner_set_strict): 'ties' (default; 'start' is its "
                        "old name) for reads with a structural tie -- two neighbouring columns with the same emission "
                        "parameters, e.g. polyA pad + A --, 'all' for every read (1.3-1.4x), 'off' for none")
    p.add_argument("--host-preprocess", action="store_true", help="normalise + Hampel-filter with NumPy on the host instead of on the GPU (same bytes)")
    p.add_argument("--event-stats", action="store_true",
                   help="add level_mean,level_stdv,level_median to every row: mean, population standard deviation and median "
                        "of the segment's samples of the normalised signal, in the model's units (computed on the GPU)")
    p.add_argument("--segment-scores", type=int, default=0, choices=range(0, 257), metavar="W",
                   help="add median_delta,mad_delta,homogeneity to every row (after the level columns, if any): the change of the "
                        "median and of the median absolute deviation between the W samples (1 .. 256, default 0 = off) before and "
                        "after the segment's first sample, and the MAD of the segment with 10 %% trimmed from either end (nan "
                        "below 10 samples; the deltas are nan in a read's first row) -- the segmentation scores of the reference's "
                        "compareTools.py, on the normalised signal, computed on the GPU")
    p.add_argument("--border-confidence", type=int, default=0, choices=range(0, 257), metavar="W",
                   help="add border_probability,border_window_probability to every row (after the level and score columns, if "
                        "any): the posterior probability, over all segmentations, that the segment starts exactly at the called "
                        "sample, and that it starts within W samples (1 .. 256, default 0 = off) of it -- computed on the GPU from "
                        "the forward-backward lattice of the alignment")
    p.add_argument("--posterior-samples", type=int, default=0, choices=range(0, 65), metavar="K",
                   help="add sample_starts to every row (after the level, score and border columns, if any): K (1 .. 64, default 0 "
                        "= off) alternative starts of the segment joined by ';', one from each of K complete segmentations of the "
                        "read drawn on the GPU from the posterior distribution over alignments -- column k of the field, read down "
                        "a read's rows, is one jointly consistent segmentation. Reproducible for the same input order, "
                        "--batch-reads and --sample-seed. Not together with --rescale-iters, --guide-auto or --guide-rescue")
    p.add_argument("--border-interval", type=float, default=0.0, metavar="MASS",
                   help="add border_lo, border_hi, border_mean, border_sd to every row (after every other optional column): the "
                        "central credible interval of posterior mass MASS (0.01 .. 0.999, default 0 = off) of the segment's start, "
                        "and the mean and standard deviation of that posterior, in the unit of the start column -- computed on the "
                        "GPU from the forward-backward lattice of the alignment. Not together with --border-confidence, "
                        "--posterior-samples, --guide-auto or --guide-rescue")
    p.add_argument("--soft-levels", action="store_true",
                   help="add soft_dwell, soft_mean, soft_stdv to every row (after every other optional column): the expected number "
                        "of samples of the base and the mean and standard deviation of the normalised signal, weighted by the "
                        "posterior that a sample belongs to the base instead of cut at the called borders -- computed on the GPU "
                        "from the forward-backward lattice of the alignment. The library refuses it together with "
                        "--border-confidence, --posterior-samples, --border-interval, --guide-auto or --guide-rescue")
    p.add_argument("--sample-seed", type=int, default=0, metavar="S", help="with --posterior-samples: the seed of the draws (default 0)")
    p.add_argument("--rescale-iters", type=int, default=0, choices=range(0, 9), metavar="N",
                   help="align every read N + 1 times (0 .. 8, default 0 = off), refitting the read's signal shift and scale "
                        "on the GPU between the passes: a least-squares fit of the segment levels on the model levels. "
                        "The rows are those of the last pass (with --event-stats, its levels). The CSV columns are unchanged; "
                        "the per-read shift and scale are not written anywhere")
    p.add_argument("--site-summary", default="", metavar="FILE",
                   help="per reference position across reads (the basecalls must be a MAPPED .bam): coverage, dwell and level "
                        "mean / sd of the reads' event means, summed on the GPU as exact integers, written as a TSV of the sites "
                        "with coverage > 0 in reference order (INTEGRATION.md section 3). One process only")
    p.add_argument("--site-capacity", type=int, default=0, metavar="ROWS",
                   help="with --site-summary FILE: keep the per-site table SPARSE, ROWS rows behind a hash map on the GPU from "
                        "reference position to row (60 bytes per row, plus the histograms' per row), instead of one row per "
                        "reference position: for genomes and transcriptomes whose dense table does not fit. Choose ROWS at least "
                        "twice the positions the reads cover. A position that finds no row in a full map is left out of FILE as a "
                        "whole (every position in FILE is complete); the run then says so and ends with exit status 3. With "
                        "--site-control the rows hold the control's positions too: a control that does not fit ends the run with a "
                        "MemoryError before any read is aligned")
    p.add_argument("--site-histogram", default="", metavar="BINS[:LO:HI]",
                   help="with --site-summary FILE: also count, per reference position, a histogram of the reads' event means with "
                        "BINS (2 .. 254) bins over [LO, HI) and one of their dwell on the GPU, and add the columns level_q25, "
                        "level_median and level_q75 to FILE, found from the histograms on the GPU. Without LO:HI the range is "
                        "the model's lowest and highest k-mer level widened by four of its largest standard deviations")
    p.add_argument("--site-table-out", default="", metavar="TABLE.npz",
                   help="with --site-summary FILE: also save the run's per-site table (and, with --site-histogram, its histograms) "
                        "as exact integers once the pipeline is dry: the covered sites as sparse columns in an .npz, for a later "
                        "run's --site-control")
    p.add_argument("--site-merge-ranks", action="store_true",
                   help="with --site-summary FILE under torch.distributed.run: every rank fills a per-site table of its own (with "
                        "--site-capacity: a sparse one of that capacity each); once the pipeline is dry the ranks pack the covered "
                        "positions on their GPUs, the records travel to rank 0, which adds them into its table by key (exact integers: "
                        "the same bits for any number of ranks) and writes every per-site output. In one process it does nothing")
    p.add_argument("--site-table-in", action="append", default=[], metavar="TABLE.npz",
                   help="with --site-summary FILE: add a table an earlier run saved with --site-table-out (the same references, the "
                        "same histogram bins and range) into this run's table before the first batch, totals included: several "
                        "flow cells of one sample add up. Repeatable")
    p.add_argument("--site-control", default="", metavar="TABLE.npz",
                   help="with --site-summary FILE and --site-histogram: compare the run, per reference position, against the table a "
                        "control run saved with --site-table-out (the same references, the same histogram bins and range, bit for "
                        "bit). FILE gains control_coverage, ks_d, ks_p, ks_level, ks_side, dwell_ks_d, welch_t and welch_df: a "
                        "binned Kolmogorov-Smirnov statistic found on the GPU from both histograms, and Welch's t from both tables")
    p.add_argument("--site-mixture", type=int, nargs="?", const=128, default=0, metavar="MAX_ITERS",
                   help="with --site-summary FILE and --site-histogram: fit, per reference position, a mixture of two Gaussians to "
                        "the level histogram by EM on the GPU (at most MAX_ITERS rounds, 1 .. 1024, default 128). FILE gains mix_share "
                        "(the share of the run's rows in the upper component), mix_mu0, mix_mu1, mix_sd0, mix_sd1, mix_iters and "
                        "mix_status; with --site-control the run and the control are pooled for the fit and mix_control_share, "
                        "mix_delta, mix_lor and mix_p compare their shares")
    p.add_argument("--site-model-out", default="", metavar="MODEL.npz",
                   help="with --site-mixture: save the fitted per-site model (the positions whose fit converged or reached MAX_ITERS: "
                        "pi1, mu0, mu1, var0, var1) with the BAM header's references and the histogram's bins and range, for a later "
                        "run's --site-model")
    p.add_argument("--site-model", default="", metavar="MODEL.npz",
                   help="with --site-summary FILE: load a per-site model saved by --site-model-out onto the GPU before the first batch "
                        "and score every row against its position's model there: every row of the output gains site_probability (the "
                        "posterior probability of the upper component, given the row's level) and site_z (the level as a z-score under "
                        "the lower component); nan where the position has no model or the read no mapping. Works with "
                        "--site-capacity: model rows that find no row in the table are reported on stderr")
    p.add_argument("--kmer-summary", default="", metavar="PATH",
                   help="also write a per-k-mer summary of the run to PATH: a TSV in the model file's k-mer order with the "
                        "level (mean, stdev of the normalised signal) and dwell the run's segments showed per k-mer beside the "
                        "model's values, summed on the GPU as exact integers (the same bytes for any number of GPUs). Its "
                        "first three columns load as a model file; k-mers the run never met keep the model's values")
    p.add_argument("--band-report", default="", metavar="FILE",
                   help="also write FILE, a TSV with one line per read the aligner took: readid, T (signal samples + 1), N "
                        "(k-mers + 1), band, band_margin_low, band_margin_high, band_edge_rows -- how close the called path came "
                        "to a real edge of its band (the smallest distance in columns below and above; empty where that edge was "
                        "never a real one or the read failed) and on how many rows it sat on one. A margin of 0 says that the band "
                        "may have decided the alignment: run those reads again with a larger --band. Lines are sorted by readid "
                        "(the same bytes for any number of GPUs); the CSV is unchanged")
    p.add_argument("--band", type=int, default=400, metavar="COLUMNS",
                   help="band width of the alignment lattice in columns (default 400, the reference's; up to 4093)")
    p.add_argument("--guide-auto", type=int, default=0, metavar="HW",
                   help="align inside a window of HW lattice columns on either side of a guide made on the GPU from the signal and "
                        "the sequence alone (no move table needed); not together with --rescale-iters or --border-confidence "
                        "(0: off)")
    p.add_argument("--guide-rounds", type=int, default=8, metavar="R",
                   help="with --guide-auto / --guide-rescue: alignments per read at the most while its guide is refined (1 .. 64)")
    p.add_argument("--guide-rescue", type=int, default=0, metavar="HW",
                   help="align every read as usual, then align again -- inside a window of HW lattice columns on either side of a "
                        "guide made on the GPU, as --guide-auto does -- only the reads whose band margin is below "
                        "--guide-rescue-margin: the cost of the plain run plus the flagged reads. A read the plain alignment "
                        "failed is not rescued. Not together with --guide-auto, --rescale-iters or --border-confidence (0: off)")
    p.add_argument("--guide-rescue-margin", type=int, default=1, metavar="M",
                   help="with --guide-rescue: a read is flagged when the smaller of its two band margins (--band-report) is "
                        "below M (default 1: the path touched a real edge of the band)")
    p.add_argument("--parallel-zstd-frames", action="store_true",
                   help="write the CSV as consecutive independent zstd frames (readers must read across frames: "
                        "python-zstandard's defaults stop after the first). Default: one frame, like the reference, "
                        "compressed on several threads either way")
    args = p.parse_args(argv)
    if args.guide_auto and args.rescale_iters:
        p.error("--guide-auto and --rescale-iters are mutually exclusive")
    if args.guide_auto and args.border_confidence:
        p.error("--guide-auto and --border-confidence are mutually exclusive")
    for other, name in ((args.guide_auto, "--guide-auto"), (args.rescale_iters, "--rescale-iters"), (args.border_confidence, "--border-confidence")):
        if args.guide_rescue and other:
            p.error("--guide-rescue and %s are mutually exclusive" % name)
    for other, name in ((args.guide_auto, "--guide-auto"), (args.rescale_iters, "--rescale-iters"), (args.guide_rescue, "--guide-rescue")):
        if args.posterior_samples and other:
            p.error("--posterior-samples and %s are mutually exclusive" % name)
    if args.border_interval != 0 and not 0.01 <= args.border_interval <= 0.999:
        p.error("--border-interval must be 0 or 0.01 .. 0.999")
    for other, name in ((args.border_confidence, "--border-confidence"), (args.posterior_samples, "--posterior-samples"),
                        (args.guide_auto, "--guide-auto"), (args.guide_rescue, "--guide-rescue")):
        if args.border_interval and other:
            p.error("--border-interval and %s are mutually exclusive" % name)
    if args.sample_seed < 0 or args.sample_seed >= 1 << 64:
        p.error("--sample-seed must be 0 .. 2^64 - 1")
    return args


def listener(q, outfile: str, header: bytes = CSV_HEADER) -> None:
    """Writer (segment.py:69-107): header, then bytes -> CSV stream, str -> ``<out>.errors``,
    "kill" terminates."""
    errfile = splitext(splitext(outfile)[0])[0] + ".errors"
    num_err = 0
    with open(outfile, "wb") as raw:
        with open_writer(raw, level=3, threads=ZSTD_WORKERS, parallel_frames=ZSTD_PARALLEL_FRAMES) as output:
            output.write(header)
            while True:
                result = q.get()
                if isinstance(result, str) and result == "kill":
                    break
                if isinstance(result, str):
                    with open(errfile, "a") as err:
                        err.write(result + "\n")
                    num_err += 1
                else:
                    output.write(result)
    print("Done segmenting reads.", file=sys.stderr)


def close_raw_cache():
    """segment.py:109-120"""
    global RAW_CACHE
    if RAW_CACHE is None:
        return
    while RAW_CACHE:
        _, reader = RAW_CACHE.popitem(last=False)
        try:
            reader.close()
        except Exception:  # noqa: BLE001
            pass


def get_raw(path):
    """LRU of RAW_CACHE_SIZE open readers (segment.py:123-139)."""
    global RAW_CACHE
    if RAW_CACHE is None:
        RAW_CACHE = OrderedDict()
    if path in RAW_CACHE:
        RAW_CACHE.move_to_end(path)
        return RAW_CACHE[path]
    if len(RAW_CACHE) >= RAW_CACHE_SIZE:
        _, old = RAW_CACHE.popitem(last=False)
        try:
            old.close()
        except Exception:  # noqa: BLE001
            pass
    RAW_CACHE[path] = open_pod5(path)
    return RAW_CACHE[path]


def generate_jobs(dataPath: str, basecalls: str, minQual: float = 0, rank: int = 0, world: int = 1):
    """(rawFile, shift, scale, start, end, sequence, readid, signalid) per basecalled read
    (segment.py:189-258): ``qs`` filter, ``pi`` parent id, ``start = sp+ts``, ``end = sp+ns``,
    file ``fn`` or ``f5``, normalisation tags ``sm``/``sd``. ``rank`` / ``world``: of the jobs that pass the filter only
    those with index % world == rank (every rank of a multi-GPU run walks the basecalls and keeps its share)."""
    skipped = 0
    if _native_bam(basecalls):  # the same walk in native code (csrc/bam_reader.cpp), re-yielded read by read
        for jb in job_batches(basecalls, minQual, 4096, False, rank, world):
            for i in range(jb.n):
                yield (join(dataPath, jb.files[jb.file_id[i]]), float(jb.shift[i]), float(jb.scale[i]), int(jb.start[i]), int(jb.end[i]),
                       jb.read(i), jb.name(i), jb.sid(i))
        return
    index = -1
    for rec in iter_basecalls(basecalls):
        qs = rec.get_tag("qs")
        if minQual and qs < minQual:
            skipped += 1
            continue
        index += 1
        if index % world != rank:
            continue
        readid = rec.query_name
        signalid = rec.get_tag("pi") if rec.has_tag("pi") else readid
        ns = rec.get_tag("ns")
        ts = rec.get_tag("ts")
        sp = rec.get_tag("sp") if rec.has_tag("sp") else 0
        raw_file = join(dataPath, rec.get_tag("fn")) if rec.has_tag("fn") else join(dataPath, rec.get_tag("f5"))
        yield (raw_file, rec.get_tag("sm"), rec.get_tag("sd"), sp + ts, sp + ns, rec.query_sequence, readid, signalid)
    print(f"Skipped reads due to low quality: {skipped}", file=sys.stderr)


def available_cpus() -> int:
    """CPUs this process may use: the affinity mask, cut down to the cgroup's CPU quota when there is one"""
    import os
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(quota) // int(period)))
    except (OSError, ValueError):
        pass
    return n


def _native_bam(basecalls: str) -> bool:
    """BAM basecalls go through the native reader unless DYN_PY_BAM=1 asks for the Python parsers (pysam when present,
    bam_io.iter_bam otherwise; tests compare the two)"""
    import os
    return basecalls.endswith(".bam") and os.environ.get("DYN_PY_BAM", "0") != "1"


def batch_site_ids(jb, aln: dict, offsets, is_rna: bool) -> tuple:
    """--site-summary: (per-read uint32 ids in aligner orientation, reads left without ids) of one JobBatch from its mapping
    (NativeBamJobs.alignment()). A read gets no ids -- DYN_SITE_NONE throughout -- when it is unmapped, secondary or
    supplementary, on the reverse strand (the stored sequence is then the reverse complement, which the pipeline aligns as it
    stands), carries its CIGAR in a CG tag (the record holds the kSmN placeholder), or has a CIGAR that does not cover it."""
    from dynamont_amd.sites import DYN_SITE_NONE, site_ids_from_cigar, to_aligner_orientation
    out, without = [], 0
    seq_len = np.diff(jb.seq_off.astype(np.int64))
    for i in range(jb.n):
        flag, ref, l_seq = int(aln["flag"][i]), int(aln["ref_id"][i]), int(jb.bases[i])
        words = aln["cigar"][int(aln["cigar_off"][i]):int(aln["cigar_off"][i + 1])]
        ids = None
        placeholder = len(words) == 2 and int(words[0]) == (l_seq << 4 | 4) and int(words[1]) & 0xF == 3
        if not flag & (0x4 | 0x10 | 0x100 | 0x800) and 0 <= ref < len(offsets) - 1 and len(words) and not placeholder:
            try:
                ids = to_aligner_orientation(site_ids_from_cigar(int(aln["pos"][i]), words, l_seq, int(offsets[ref])), is_rna,
                                             int(seq_len[i]) - l_seq)
            except ValueError:
                ids = None
        if ids is None:
            without += 1
            ids = np.full(int(seq_len[i]), DYN_SITE_NONE, dtype=np.uint32)
        out.append(ids)
    return out, without


def job_batches(basecalls: str, minQual: float, batch_reads: int, is_rna: bool, rank: int = 0, world: int = 1, site_offsets=None,
                site_counts=None):
    """generate_jobs a batch at a time, as columns (bam_io.JobBatch): the quality filter, the rank's share
    (index % world == rank) and -- ``is_rna`` -- the workers' sequence orientation (segment.py:149-153) are applied by the
    native reader. ``site_offsets`` (--site-summary: sites.contig_offsets of the header's references): every batch carries
    ``site_ids``, and ``site_counts`` [reads, reads left without ids] is added to."""
    from dynamont_amd.bam_io import NativeBamJobs
    reader = NativeBamJobs(basecalls, rna=is_rna, pad=POLYA, min_qual=minQual or 0.0, rank=rank, world=world)
    try:
        while True:
            jb = reader.next(batch_reads)
            if jb is None:
                break
            if site_offsets is not None:
                jb.site_ids, without = batch_site_ids(jb, reader.alignment(), site_offsets, is_rna)
                if site_counts is not None:
                    site_counts[0] += jb.n
                    site_counts[1] += without
            yield jb
        print(f"Skipped reads due to low quality: {reader.skipped}", file=sys.stderr)
    finally:
        reader.close()


def _ragged(starts: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """[starts[0], starts[0]+1, .. starts[0]+counts[0]-1, starts[1], ..] as one int64 array"""
    counts = counts.astype(np.int64)
    total = int(counts.sum())
    first = np.cumsum(counts) - counts
    return np.arange(total, dtype=np.int64) - np.repeat(first, counts) + np.repeat(starts.astype(np.int64), counts)


def prepare_job_columns(jb, data_path: str, put_error):
    """prepare_job_raw for a whole JobBatch whose raw files can point at their compressed chunks
    (pod5_native.Pod5File.signal_chunks_batch). Returns (jb, chunks, raw_off, cal, owners): ``jb`` without the reads that
    failed (each reported through ``put_error`` with the worker's line, segment.py:178-187), ``chunks`` = (ptrs, nbytes,
    samples, read_off, slice_start) for dyn_batch_align_vbz_async, ``raw_off`` the prefix sums of the slice lengths,
    ``cal`` = (offset, scale, calibrated mask); or None when a reader of the batch cannot do that (the caller then takes
    the per-read path)."""
    import uuid as uuid_mod
    n = jb.n
    for i in np.flatnonzero(jb.uuid_ok == 0):  # ids the native parser did not take: uuid.UUID() accepts a few more spellings
        try:
            jb.uuid[i] = np.frombuffer(uuid_mod.UUID(jb.sid(i)).bytes, dtype=np.uint8)
            jb.uuid_ok[i] = 1
        except ValueError:
            pass
    found = np.zeros(n, dtype=bool)
    cnt = np.zeros(n, dtype=np.int64)
    cal_o = np.zeros(n, dtype=np.float32)
    cal_s = np.zeros(n, dtype=np.float32)
    parts, owners, failed = [], [], {}
    for fid, fname in enumerate(jb.files):
        sel = np.flatnonzero(jb.file_id == fid)
        if not len(sel):
            continue
        try:
            reader = get_raw(join(data_path, fname))
            fn = getattr(reader, "signal_chunks_batch", None)
            res = fn(jb.uuid[sel]) if fn is not None else None
        except Exception as error:  # noqa: BLE001  the file cannot be opened or read: every read of it fails like in the worker
            for i in sel:
                failed[int(i)] = error
            continue
        if res is None:
            return None
        ok, ptrs, nbytes, samples, roff, co, cs = res
        ok = ok & (jb.uuid_ok[sel] != 0)
        if not ok.all():  # (chunks of reads that were found under a damaged id cannot exist: ok False implies no chunks, or drop them)
            keep_chunks = np.repeat(ok, np.diff(roff.astype(np.int64)))
            ptrs, nbytes, samples = ptrs[keep_chunks], nbytes[keep_chunks], samples[keep_chunks]
        c = np.where(ok, np.diff(roff.astype(np.int64)), 0)
        found[sel], cnt[sel], cal_o[sel], cal_s[sel] = ok, c, co, cs
        parts.append((sel, c, ptrs, nbytes, samples))
        owners.append(reader)
    for i in np.flatnonzero(~found):
        i = int(i)
        error = failed.get(i, KeyError(jb.sid(i)))
        put_error(f"error: worker, {error}\tN: {int(jb.bases[i])}\tRid: {jb.name(i)}\tSid: {jb.sid(i)}")
    read_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(cnt, out=read_off[1:])
    total = int(read_off[-1])
    if len(parts) == 1 and found.all():
        _, _, ptrs, nbytes, samples = parts[0]
    else:  # several raw files in one batch: each file's chunks go to its reads' places
        ptrs, nbytes, samples = np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint64), np.zeros(total, dtype=np.uint32)
        for sel, c, p_, b_, s_ in parts:
            pos = _ragged(read_off[:-1][sel], c)
            ptrs[pos], nbytes[pos], samples[pos] = p_, b_, s_
    if not found.all():
        keep = np.flatnonzero(found)
        jb = jb.take(keep)
        cnt, cal_o, cal_s = cnt[keep], cal_o[keep], cal_s[keep]
        read_off = np.zeros(jb.n + 1, dtype=np.uint64)
        np.cumsum(cnt, out=read_off[1:])
    # the [start:end) slice, clipped to the read like VbzSlice clips
    csum = np.zeros(total + 1, dtype=np.int64)
    np.cumsum(samples, out=csum[1:])
    ro = read_off.astype(np.int64)
    have = csum[ro[1:]] - csum[ro[:-1]]
    s0 = np.minimum(np.maximum(jb.start, 0), have)
    e0 = np.minimum(np.maximum(jb.end, s0), have)
    raw_off = np.zeros(jb.n + 1, dtype=np.uint64)
    np.cumsum(e0 - s0, out=raw_off[1:])
    calibrated = jb.shift <= 400  # segment.py:147: the picoampere signal for these reads, the ADC counts otherwise
    return jb, (ptrs, nbytes, samples, read_off, s0.astype(np.uint64)), raw_off, (cal_o, cal_s, calibrated), owners


def jobs_from_columns(jb, data_path: str):
    """the per-read job tuples of a JobBatch (sequences as the batch holds them: already oriented when it was read so)"""
    return [(join(data_path, jb.files[jb.file_id[i]]), float(jb.shift[i]), float(jb.scale[i]), int(jb.start[i]), int(jb.end[i]),
             jb.read(i), jb.name(i), jb.sid(i)) for i in range(jb.n)]


def prepare_job(job, is_rna: bool):
    """P1 (segment.py:141-158): slice, float64, ``-= shift``, ``/= scale``, Hampel(3, 3 sigma);
    RNA: reverse the basecall and prepend the polyA pad unless present."""
    raw_file, shift, scale, start, end, read, readid, signalid = job
    r5 = get_raw(raw_file)
    signal = np.array(get_signal(r5, signalid, calibrated=shift <= 400)[start:end], dtype=np.float64, copy=True)
    signal -= shift
    signal /= scale
    hampel(signal)
    if is_rna:
        read = read[::-1]
        if not read.startswith(POLYA):
            read = POLYA + read
    return signal, read


BAND_REPORT_HEADER = b"readid\tT\tN\tband\tband_margin_low\tband_margin_high\tband_edge_rows\n"


def band_report_lines(readids, T, N, band, low, high, edge_rows) -> list:
    """--band-report: one line (no newline) per read; an empty field for DYN_BAND_MARGIN_NONE. ``band``: one width for every
    read, or one per read (--guide-rescue: a rescued read's margins are those against its guided window)"""
    none = 0xFFFFFFFF
    field = lambda v: "" if int(v) == none else str(int(v))  # noqa: E731
    bands = [int(band)] * len(readids) if np.ndim(band) == 0 else band
    return [f"{rid}\t{int(t)}\t{int(n)}\t{int(b)}\t{field(lo)}\t{field(hi)}\t{int(e)}"
            for rid, t, n, b, lo, hi, e in zip(readids, T, N, bands, low, high, edge_rows)]


def band_report_bytes(lines) -> bytes:
    """the report file: the header, then the lines sorted (by readid first: the order does not depend on batches or ranks)"""
    return BAND_REPORT_HEADER + "".join(ln + "\n" for ln in sorted(lines)).encode()


def _report_band(aligner, rescue=None):
    """the ``band`` column of --band-report: under --guide-auto the margins are those against the guided window, 2 * HW wide;
    under --guide-rescue (``rescue``: the ticket's per-read codes) those of the rescued reads are, the others' the band's"""
    if rescue is not None and aligner._guide_rescue[1]:
        return np.where(np.asarray(rescue) == 1, 2 * aligner._guide_rescue[1], aligner.band)
    return 2 * aligner._auto_guide[0] if aligner._auto_guide[0] else aligner.band


def _rescue_codes(t):
    """--guide-rescue: the per-read codes of a COMPLETED ticket (None for a ticket submitted without the switch)"""
    if not t._wants.rescue:
        return None
    t.result._fetch_one(t._L, t._h, t._al, "rescue", True)
    return t.result.rescue


def _rescue_counts(t, codes) -> tuple:
    """--guide-rescue: (flagged, rescued, rescued without converging, left for want of memory, left because the rescue failed)"""
    codes = np.asarray(codes)
    open_ = (codes == 1) & (np.asarray(t.result.guide_converged) == 0)
    return int((codes != 0).sum()), int((codes == 1).sum()), int(open_.sum()), int((codes == 2).sum()), int((codes == 3).sum())


def _guide_counts(t) -> tuple:
    """--guide-auto: (reads aligned inside their own guide, those of them whose guide did not converge) of a COMPLETED ticket"""
    from dynamont_amd._dynamont import Batch
    ok = np.asarray(t.result.status[:t.result.n]) == 0
    _, converged = Batch.guide_rounds(t)
    return int(ok.sum()), int((ok & (converged == 0)).sum())


def _ticket_band_lines(aligner, t, readids, lengths, seq_off, rescue=None) -> list:
    """the report lines of a COMPLETED align ticket submitted with the band-margin switch on"""
    from dynamont_amd import _native as N
    n = len(readids)
    low, high, edge = (np.zeros(n, dtype=np.uint32) for _ in range(3))
    t.fetch_band_margin(N.DynBandMarginOut(low.ctypes.data_as(N.c_u32_p), high.ctypes.data_as(N.c_u32_p),
                                           edge.ctypes.data_as(N.c_u32_p), n))
    bases = np.diff(np.asarray(seq_off, dtype=np.int64))
    cols = np.maximum(bases - aligner.kmer_size + 1, 0) + 1
    return band_report_lines(readids, np.asarray(lengths, dtype=np.int64) + 1, cols, _report_band(aligner, rescue), low, high, edge)


def _stored_bases(p) -> int:
    """bases of the basecall as the BAM stores it -- what the reference's worker line reports as N (segment.py:178-187).
    ``p`` = (signal, read, job, cal[, stored bases]): the fifth element where job[5] is already in aligner orientation"""
    return int(p[4]) if len(p) > 4 else len(p[2][5])


def prepare_job_raw(job, is_rna: bool, oriented: bool = False):
    """P1 without the arithmetic: the raw [start:end) slice and the aligner-orientation read. The slice is int16 ADC
    counts; ``cal`` = (offset, scale) when the reference would take the calibrated picoampere signal (``shift <= 400``,
    segment.py:147), None when it takes the ADC counts themselves. Calibration, normalisation and the Hampel filter
    then run on the device (dyn_batch_align_raw_async), bit-identically. Returns (raw, read, cal)."""
    raw_file, shift, scale, start, end, read, readid, signalid = job
    reader = get_raw(raw_file)
    chunks = get_signal_chunks(reader, signalid)
    if chunks is not None:  # a .pod5 file with VBZ chunks: they go to the library as they are (decoded on its helper threads)
        ptrs, nbytes, samples, cal_offset, cal_scale = chunks
        raw = VbzSlice(ptrs, nbytes, samples, start, end, owner=reader)
    else:
        adc, cal_offset, cal_scale = get_signal_adc(reader, signalid)
        raw = adc[start:end]
        if raw.dtype != np.int16:  # a reader that hands out something else: through the generic float64 path
            raw = raw.astype(np.float64)
    if is_rna and not oriented:  # (``oriented``: the job comes from a JobBatch that was read in aligner orientation)
        read = read[::-1]
        if not read.startswith(POLYA):
            read = POLYA + read
    return raw, read, ((cal_offset, cal_scale) if shift <= 400 and raw.dtype == np.int16 else None)


class _Collector:
    """Queue-like sink used by the non-root ranks of a multi-GPU run: rows and error lines of one
    round are collected and shipped to rank 0 (BASELINE.json config 4: gather of per-read CSV rows)."""

    def __init__(self):
        self.rows, self.errors = [], []

    def put(self, item):
        (self.errors if isinstance(item, str) else self.rows).append(item)

    def drain(self):
        r, e = b"".join(self.rows), "\n".join(self.errors).encode()
        self.rows, self.errors = [], []
        return r, e


def _pack_jobs(pending, scattered: bool = False):
    """(signal slices, reads, jobs) of one batch -> the packed arrays of the C ABI. ``scattered``: the slices stay
    where they are (a list of arrays; the library gathers them into its pinned staging buffer on its own threads)."""
    n = len(pending)
    sig_off = np.zeros(n + 1, dtype=np.uint64)
    seq_off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum([len(p[0]) for p in pending], out=sig_off[1:])
    np.cumsum([len(p[1]) for p in pending], out=seq_off[1:])
    if n and getattr(pending[0][0], "vbz", False):  # compressed POD5 chunks: flattened chunk tables
        counts = [len(p[0].ptrs) for p in pending]
        read_off = np.zeros(n + 1, dtype=np.uint64)
        np.cumsum(counts, out=read_off[1:])
        sig = (np.concatenate([p[0].ptrs for p in pending]), np.concatenate([p[0].nbytes for p in pending]),
               np.concatenate([p[0].samples for p in pending]), read_off, np.array([p[0].start for p in pending], dtype=np.uint64))
    elif scattered:
        sig = [p[0] for p in pending]
    else:
        sig = np.concatenate([p[0] for p in pending]) if n else np.zeros(0, dtype=np.int16)
    seqs = "".join(p[1] for p in pending).encode("latin-1")
    return sig, sig_off, seqs, seq_off


class _Pipeline:
    """The GPU side of dynamont-resquiggle as a stream of batches (the reference keeps a pool of worker processes
    permanently fed, segment.py:296-325): the caller's thread reads and slices batch k+1 while up to ``depth``
    batches are inside the asynchronous engine (dyn_batch_align_raw_async: staging, H2D, normalise + Hampel, the
    read queue, D2H, unpacking -- all overlapped between neighbouring batches), and ONE consumer thread waits for
    the oldest batch, formats its rows natively (dyn_format_csv, bytes == utils.segmentation_to_string) and hands
    them to the sink, under the kernels of the batches behind it. Python only moves references; every heavy call
    releases the GIL."""

    def __init__(self, aligner: Aligner, sink, raw: bool, depth: int = 3, threads: int = 8):
        self.aligner, self.sink, self.raw, self.threads = aligner, sink, raw, threads
        self.inflight = queue_mod.Queue(maxsize=max(1, depth))
        self.free = []            # result objects of completed batches, refilled instead of reallocated
        self.band_lines = []      # --band-report: the lines of the tickets completed so far
        self.guide_counts = [0, 0]  # --guide-auto: reads aligned inside their own guide, reads whose guide did not converge
        self.rescue_counts = [0, 0, 0, 0, 0]  # --guide-rescue: _rescue_counts, summed over the tickets
        self.error = None
        self.rounds_done = queue_mod.Queue()
        self.consumer = threading.Thread(target=self._drain, daemon=True)
        self.consumer.start()

    def submit(self, pending, end_of_round: bool = False) -> None:
        """Queue one batch (blocks while ``depth`` batches are in flight). Batches whose raw slices have different
        dtypes (float32 pA vs int16 ADC, segment.py:147) go up as one submission per dtype."""
        self.check()
        groups = [pending]
        if self.raw and pending:  # one submission per kind of raw data: calibrated ADC, plain ADC, anything else
            kind = lambda p: (p[0].dtype.str, p[3] is not None, getattr(p[0], "vbz", False))  # noqa: E731
            kinds = sorted({kind(p) for p in pending})
            if len(kinds) > 1:
                groups = [[p for p in pending if kind(p) == kd] for kd in kinds]
        for g in groups:
            if not g:
                continue
            sig, sig_off, seqs, seq_off = _pack_jobs(g, scattered=self.raw)
            out = self.free.pop() if self.free else None
            if self.raw:
                cal = ([p[3][0] for p in g], [p[3][1] for p in g]) if g[0][3] is not None else None
                submit_raw = self.aligner.align_vbz_async if isinstance(sig, tuple) else self.aligner.align_raw_async
                t = submit_raw(sig, sig_off, [p[2][1] for p in g], [p[2][2] for p in g], seqs, seq_off,
                               window=3, n_sigmas=3.0, f32=False, calc_probabilities=True, out=out, calibration=cal)
            else:
                t = self.aligner.align_async(sig, sig_off, seqs, seq_off, True, out=out)
            self.inflight.put((t, g, seqs, seq_off))
        if end_of_round:
            self.inflight.put("round")

    def check(self) -> None:
        if self.error is not None:
            raise self.error

    def wait_round(self) -> None:
        self.rounds_done.get()
        self.check()

    def close(self) -> None:
        """Everything submitted has been formatted and handed to the sink when this returns."""
        self.inflight.put(None)
        self.consumer.join()
        self.check()

    def _finish(self, t, g, seqs, seq_off) -> None:
        from dynamont_amd._dynamont import format_csv
        res = t.wait()
        if self.aligner._auto_guide[0]:
            for k, v in enumerate(_guide_counts(t)):
                self.guide_counts[k] += v
        codes = _rescue_codes(t)
        if codes is not None:
            for k, v in enumerate(_rescue_counts(t, codes)):
                self.rescue_counts[k] += v
        if self.aligner._band_margin:
            self.band_lines += band_report_lines([p[2][6] for p in g], [len(p[0]) + 1 for p in g],
                                                 np.maximum(np.diff(np.asarray(seq_off, dtype=np.int64)) - self.aligner.kmer_size + 1, 0) + 1,
                                                 _report_band(self.aligner, codes), res.band_margin_low, res.band_margin_high, res.band_edge_rows)
        starts = [p[2][3] for p in g]
        buf, begin, end = format_csv(self.aligner, res, None, [p[2][6] for p in g], [p[2][7] for p in g], starts,
                                     [len(p[0]) + st for p, st in zip(g, starts)], threads=self.threads, compact=True,
                                     seqs_packed=(seqs, seq_off))
        total = int(end[-1]) if len(end) else 0
        if total:
            self.sink.put(buf[:total].tobytes())
        for i in np.flatnonzero(res.status[:len(g)] != 0):
            signal, read, job = g[i][:3]
            if int(res.status[i]) == 10:  # DYN_READ_BAD_SIGNAL: the reference's worker fails before the aligner (segment.py:178-187)
                self.sink.put(f"error: worker, {res.error(i)}\tN: {_stored_bases(g[i])}\tRid: {job[6]}\tSid: {job[7]}")
                continue
            self.sink.put(f"error: native, {res.error(i)}\tT: {len(signal)}\tN: {len(read)}\tRid: {job[6]}\tSid: {job[7]}")
        t.close()
        self.free.append(res)

    def _drain(self) -> None:
        while True:
            item = self.inflight.get()
            if item is None:
                return
            if isinstance(item, str):
                self.rounds_done.put(True)
                continue
            try:
                if self.error is None:
                    self._finish(*item)
                else:
                    item[0].close()  # after a failure: only release what is still queued
            except BaseException as e:  # noqa: BLE001  (re-raised on the submitting thread)
                self.error = e
                try:
                    item[0].close()
                except Exception:  # noqa: BLE001
                    pass


class _NativePipeline:
    """Single-process form of :class:`_Pipeline` with the whole back half native (csv_sink.cpp): a batch is handed to
    dyn_batch_align_raw_async and its ticket straight on to the library's CSV sink, whose threads wait for it, format,
    compress into the one zstd frame and write -- Python only builds the next batch. Same interface as _Pipeline."""

    def __init__(self, aligner: Aligner, outfile: str, raw: bool, depth: int = 3, threads: int = 8, first: bool = True,
                 last: bool = True, errfile: str | None = None, level: int = 3):
        """``first`` / ``last``: this process writes a PART of the frame (dyn_csv_sink_open_part: one process per GPU, every
        rank compresses its own rows) -- with the header line and the frame header / with the frame's closing block."""
        import ctypes as C
        from dynamont_amd import _native as N
        self.C, self.N, self.L = C, N, N.lib()
        self.aligner, self.raw, self.depth = aligner, raw, max(1, depth)
        errfile = errfile or splitext(splitext(outfile)[0])[0] + ".errors"
        h = C.c_void_p()
        err = C.create_string_buffer(1024)
        import os
        threads = int(os.environ.get("DYN_SINK_THREADS", threads))
        self.threads = threads
        flags = N.DYN_CSV_EVENT_STATS if aligner._event_stats else 0  # the rows carry the signal levels (--event-stats)
        if aligner._segment_scores:
            flags |= N.DYN_CSV_SEGMENT_SCORES  # ... and the segment scores (--segment-scores)
        if aligner._border_confidence:
            flags |= N.DYN_CSV_BORDER_CONFIDENCE  # ... and the border confidence (--border-confidence)
        if aligner._posterior_samples[0]:
            flags |= N.DYN_CSV_POSTERIOR_SAMPLES  # ... and the posterior samples (--posterior-samples)
        if aligner._border_interval:
            flags |= N.DYN_CSV_BORDER_INTERVAL  # ... and the credible intervals (--border-interval)
        if aligner._soft_levels:
            flags |= N.DYN_CSV_SOFT_LEVELS  # ... and the soft levels (--soft-levels)
        if aligner._site_calls:
            flags |= N.DYN_CSV_SITE_CALLS  # ... and the site calls (--site-model)
        rc = self.L.dyn_csv_sink_open_ex(outfile.encode(), errfile.encode(), int(os.environ.get("DYN_SINK_LEVEL", level)), int(threads),
                                         int(first), int(last), flags, C.byref(h), err, 1024)
        if rc != N.DYN_OK:
            raise OSError(err.value.decode())
        self.h = h
        self.submitted = 0
        self.samples = {}  # batch number -> signal samples (in flight: bounded by MAX_SAMPLES_IN_FLIGHT as well as by depth)
        self.keep = {}   # batch number -> (ticket, arrays the sink still reads)
        self.free = []   # result objects of consumed batches
        self.band_meta = {}   # --band-report: batch number -> (readids, signal lengths, sequence offsets)
        self.band_lines = []  # ... and the lines of the tickets the sink has consumed
        self.guide_counts = [0, 0]  # --guide-auto: reads aligned inside their own guide, reads whose guide did not converge
        self.rescue_counts = [0, 0, 0, 0, 0]  # --guide-rescue: _rescue_counts, summed over the tickets

    def put(self, line: str) -> None:
        """an error line from the producer (reads that failed before the aligner, segment.py:178-187)"""
        if self.L.dyn_csv_sink_error_line(self.h, line.encode()) != self.N.DYN_OK:
            raise OSError("cannot append to the .errors file")

    def _reap(self, block_until: int | None = None) -> None:
        """release what the sink has consumed; ``block_until``: wait (in the library, not polling) until at most that many
        batches are in flight"""
        while True:
            done = int(self.L.dyn_csv_sink_completed(self.h))
            for k in [k for k in self.keep if k < done]:
                t, res = self.keep.pop(k)[:2]
                self.samples.pop(k, None)
                self._band_collect(k, t)
                t.close()
                self.free.append(res)
            if block_until is None or self.submitted - done <= block_until:
                return
            self.check()
            self.L.dyn_csv_sink_wait(self.h, self.submitted - block_until, 200)

    def _band_collect(self, k: int, t) -> None:
        """--band-report: the margins of a ticket the sink is done with, before the ticket goes (and --guide-auto's counts)"""
        if self.aligner._auto_guide[0]:
            for j, v in enumerate(_guide_counts(t)):
                self.guide_counts[j] += v
        codes = _rescue_codes(t)
        if codes is not None:
            for j, v in enumerate(_rescue_counts(t, codes)):
                self.rescue_counts[j] += v
        meta = self.band_meta.pop(k, None)
        if meta is not None:
            self.band_lines += _ticket_band_lines(self.aligner, t, *meta, rescue=codes)

    def submit(self, pending, end_of_round: bool = False) -> None:
        C, N = self.C, self.N
        groups = [pending]
        if self.raw and pending:
            kind = lambda p: (p[0].dtype.str, p[3] is not None, getattr(p[0], "vbz", False))  # noqa: E731
            kinds = sorted({kind(p) for p in pending})
            if len(kinds) > 1:
                groups = [[p for p in pending if kind(p) == kd] for kd in kinds]
        for g in groups:
            if not g:
                continue
            self.check()
            n = len(g)
            sig, sig_off, seqs, seq_off = _pack_jobs(g, scattered=self.raw)
            self._room_for(int(sig_off[-1]))
            out = self.free.pop() if self.free else None
            if self.raw:
                cal = ([p[3][0] for p in g], [p[3][1] for p in g]) if g[0][3] is not None else None
                # --site-summary: every pending tuple then carries its read's ids as a sixth element (all of them or none)
                ids = np.concatenate([p[5] for p in g]) if all(len(p) > 5 and p[5] is not None for p in g) else None
                submit_raw = self.aligner.align_vbz_async if isinstance(sig, tuple) else self.aligner.align_raw_async
                t = submit_raw(sig, sig_off, [p[2][1] for p in g], [p[2][2] for p in g], seqs, seq_off,
                               window=3, n_sigmas=3.0, f32=False, calc_probabilities=True, out=out, calibration=cal, site_ids=ids)
            else:
                t = self.aligner.align_async(sig, sig_off, seqs, seq_off, True, out=out)
            res = t.result
            rid = (C.c_char_p * n)(*[str(p[2][6]).encode() for p in g])
            sid = (C.c_char_p * n)(*[str(p[2][7]).encode() for p in g])
            starts = np.array([p[2][3] for p in g], dtype=np.int64)
            lengths = np.diff(sig_off).astype(np.uint64)
            bases = np.array([_stored_bases(p) for p in g], dtype=np.uint32)
            rc = self.L.dyn_csv_sink_submit_bases(self.h, self.aligner._h, t._h, C.byref(res._c), n, seqs,
                                                  seq_off.ctypes.data_as(N.c_u64_p), rid, sid,
                                                  starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(N.c_u64_p),
                                                  bases.ctypes.data_as(C.POINTER(C.c_uint32)))
            if rc != N.DYN_OK:
                t.close()
                self.check()  # the sink's own failure, with its message
                raise RuntimeError("dyn_csv_sink_submit failed")
            self.keep[self.submitted] = (t, res, seqs, seq_off, rid, sid, starts, lengths, g, bases)  # g: the slices (and their readers) stay alive
            if self.aligner._band_margin:
                self.band_meta[self.submitted] = ([str(p[2][6]) for p in g], lengths, seq_off)
            self.samples[self.submitted] = int(sig_off[-1])
            self.submitted += 1

    def _room_for(self, samples: int) -> None:
        """``depth`` batches in flight, fewer when they are large (every batch in flight holds its samples as int16 in
        pinned host memory and as float64 on the device)"""
        self._reap(block_until=self.depth - 1)
        while self.samples and sum(self.samples.values()) + samples > MAX_SAMPLES_IN_FLIGHT:
            self._reap(block_until=len(self.samples) - 1)

    def submit_columns(self, jb, chunks, raw_off, cal, owners) -> None:
        """One batch prepared by prepare_job_columns: compressed POD5 chunks and column arrays straight into
        dyn_batch_align_vbz_async and the sink -- no Python object per read. Reads with and without calibration
        (segment.py:147) go up as separate submissions, like in submit()."""
        C, N = self.C, self.N
        cal_o, cal_s, calibrated = cal
        if jb.n == 0:
            return
        if calibrated.any() and not calibrated.all():
            ptrs, nbytes, samples, read_off, skip = chunks
            cnt = np.diff(read_off.astype(np.int64))
            lens = np.diff(raw_off.astype(np.int64))
            for mask in (~calibrated, calibrated):  # (the order submit() sends its groups in)
                keep = np.flatnonzero(mask)
                pos = _ragged(read_off[:-1][keep], cnt[keep])
                ro = np.zeros(len(keep) + 1, dtype=np.uint64)
                np.cumsum(cnt[keep], out=ro[1:])
                so = np.zeros(len(keep) + 1, dtype=np.uint64)
                np.cumsum(lens[keep], out=so[1:])
                self.submit_columns(jb.take(keep), (ptrs[pos], nbytes[pos], samples[pos], ro, skip[keep]), so,
                                    (cal_o[keep], cal_s[keep], calibrated[keep]), owners)
            return
        self.check()
        self._room_for(int(raw_off[-1]))
        n = jb.n
        out = self.free.pop() if self.free else None
        ids = getattr(jb, "site_ids", None)  # --site-summary: the batch's per-read ids, packed like its sequences
        t = self.aligner.align_vbz_async(chunks, raw_off, jb.shift, jb.scale, jb.seqs, jb.seq_off, window=3, n_sigmas=3.0, f32=False,
                                         calc_probabilities=True, out=out, calibration=(cal_o, cal_s) if calibrated.all() else None,
                                         site_ids=np.concatenate(ids) if ids else None)
        res = t.result
        rid = (jb.names.ctypes.data + jb.name_off[:-1]).astype(np.uint64)  # char* of every NUL-terminated name
        sid = (jb.sids.ctypes.data + jb.sid_off[:-1]).astype(np.uint64)
        starts = np.ascontiguousarray(jb.start, dtype=np.int64)
        lengths = np.diff(raw_off).astype(np.uint64)
        seq_off = np.ascontiguousarray(jb.seq_off, dtype=np.uint64)
        bases = np.ascontiguousarray(jb.bases, dtype=np.uint32)
        rc = self.L.dyn_csv_sink_submit_bases(self.h, self.aligner._h, t._h, C.byref(res._c), n, jb.seqs, seq_off.ctypes.data_as(N.c_u64_p),
                                              C.cast(rid.ctypes.data, C.POINTER(C.c_char_p)), C.cast(sid.ctypes.data, C.POINTER(C.c_char_p)),
                                              starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(N.c_u64_p),
                                              bases.ctypes.data_as(C.POINTER(C.c_uint32)))
        if rc != N.DYN_OK:
            t.close()
            self.check()
            raise RuntimeError("dyn_csv_sink_submit failed")
        self.keep[self.submitted] = (t, res, jb, seq_off, rid, sid, starts, lengths, chunks, raw_off, cal, owners, bases)
        if self.aligner._band_margin:
            names = jb.names.tobytes()
            self.band_meta[self.submitted] = ([names[int(a):int(b) - 1].decode() for a, b in zip(jb.name_off[:-1], jb.name_off[1:])],
                                              lengths, seq_off)
        self.samples[self.submitted] = int(raw_off[-1])
        self.submitted += 1

    def check(self) -> None:
        """raise as soon as the sink has failed (a batch error, zstd, the output file) instead of parsing and aligning the
        rest of the input first; close() delivers the message"""
        if self.h is not None and self.L.dyn_csv_sink_failed(self.h):
            self.close()

    def close(self) -> None:
        C = self.C
        if self.h is None:
            return
        csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
        err = C.create_string_buffer(1024)
        _stamp("closing the sink (every batch submitted; the last tickets are on the GPU)")
        rc = self.L.dyn_csv_sink_close(self.h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024)
        _stamp("sink closed: the file is complete")
        self.h = None
        LAST_RUN.update(csv_bytes=int(csv.value), compressed_bytes=int(zst.value), error_lines=int(nerr.value), batches=self.submitted,
                        depth=self.depth, compress_threads=self.threads)
        for k, (t, *_) in self.keep.items():
            if rc == self.N.DYN_OK:
                self._band_collect(k, t)  # (the sink has waited for every ticket)
            t.close()
        self.keep = {}
        _stamp("tickets released")
        print("Done segmenting reads.", file=sys.stderr)
        if rc != self.N.DYN_OK:
            raise RuntimeError(err.value.decode())


def _gather_parts(comm, parallel, outfile: str, part: str, part_err: str | None) -> None:
    """One process per GPU, all ranks done: the parts of the frame (complete zstd blocks, compressed where their rows
    were computed) travel to rank 0 rank by rank -- a part must stay in one piece -- and are appended to its own part,
    followed by the frame's closing block; the ranks' error lines likewise. The only exchange of the job."""
    import os
    rank, world = comm.rank, comm.world
    chunk_bytes = 64 << 20
    out = open(outfile, "ab") if rank == 0 else None
    for src in range(1, world):
        f = open(part, "rb") if rank == src else None
        while True:
            chunk = f.read(chunk_bytes) if f else b""
            blobs = parallel.gather_bytes(comm, chunk)
            if rank == 0 and blobs[src]:
                out.write(blobs[src])
            if not parallel.any_rank(comm, rank == src and len(chunk) == chunk_bytes):
                break
        if f:
            f.close()
    if out:
        out.write(b"\x01\x00\x00")  # DYN_ZSTD_FRAME_END: an empty last block closes the frame
        out.close()
    text = b""
    if rank != 0 and part_err and os.path.exists(part_err):
        text = open(part_err, "rb").read()
    blobs = parallel.gather_bytes(comm, text)
    if rank == 0:
        extra = b"".join(b for b in blobs[1:] if b)
        if extra:
            with open(splitext(splitext(outfile)[0])[0] + ".errors", "ab") as f:
                f.write(extra)
    else:
        for path in (part, part_err):
            if path and os.path.exists(path):
                os.remove(path)


def segment(data_path: str, basecalls: str, processes: int, outfile: str, model_path: str, pore: str, mode: str,
            minq: float = 0, device: int = 0, batch_reads: int = 1024, mem_budget_gib: float = 0.0,
            host_preprocess: bool = False, depth: int = 12, strict_ties: str = "ties", host_threads: int = 0,
            zstd_level: int = 3, event_stats: bool = False, rescale_iters: int = 0, kmer_summary: str = "",
            segment_scores: int = 0, border_confidence: int = 0, band_report: str = "", band: int = 400,
            guide_auto: int = 0, guide_rounds: int = 8, guide_rescue: int = 0, guide_rescue_margin: int = 1,
            posterior_samples: int = 0, sample_seed: int = 0, border_interval: float = 0.0,
            soft_levels: bool = False, site_summary: str = "", site_histogram: str = "", site_table_out: str = "",
            site_control: str = "", site_mixture: int = 0, site_capacity: int = 0, site_model_out: str = "", site_model: str = "",
            site_merge_ranks: bool = False, site_table_in=()) -> None:
    """Counterpart of segment.py:261-371. Under ``torch.distributed.run`` every rank drives one GPU
    on the reads ``index % world == rank``, formats and compresses its rows into a part of the output
    frame, and the parts' bytes are gathered to rank 0, which owns the file (reads are independent;
    that gather at the end is the only exchange). ``guide_auto`` > 0: every batch is aligned inside guides the library
    makes itself at that half width, refined up to ``guide_rounds`` alignments per read (``Aligner.set_auto_guide``).
    ``guide_rescue`` > 0: every batch is aligned as usual and only the reads whose band margin is below ``guide_rescue_margin``
    are aligned again inside such a guide (``Aligner.set_guide_rescue``)."""
    if guide_auto < 0 or (guide_auto and (rescale_iters or border_confidence)):
        raise ValueError("--guide-auto must be >= 0 and is not combined with --rescale-iters or --border-confidence")
    if guide_rescue < 0 or guide_rescue_margin < 0 or (guide_rescue and (guide_auto or rescale_iters or border_confidence)):
        raise ValueError("--guide-rescue and --guide-rescue-margin must be >= 0; --guide-rescue is not combined with --guide-auto, "
                         "--rescale-iters or --border-confidence")
    if not 0 <= posterior_samples <= 64 or (posterior_samples and (guide_auto or guide_rescue or rescale_iters)):
        raise ValueError("--posterior-samples must be 0 .. 64 and is not combined with --guide-auto, --guide-rescue or --rescale-iters")
    if border_interval and (not 0.01 <= border_interval <= 0.999 or border_confidence or posterior_samples or guide_auto or guide_rescue):
        raise ValueError("--border-interval must be 0 or 0.01 .. 0.999 and is not combined with --border-confidence, "
                         "--posterior-samples, --guide-auto or --guide-rescue")
    site_hist = None
    if site_histogram:
        from dynamont_amd.segmentation.utils import parse_site_histogram
        if not site_summary:
            raise ValueError("--site-histogram counts beside the per-site table: it needs --site-summary FILE")
        site_hist = parse_site_histogram(site_histogram)
    if site_table_out and not site_summary:
        raise ValueError("--site-table-out saves the per-site table: it needs --site-summary FILE")
    if site_control and not (site_summary and site_hist):
        raise ValueError("--site-control compares the per-site histograms of the run and the control: it needs --site-summary FILE and "
                         "--site-histogram BINS[:LO:HI]")
    if site_mixture and not (site_summary and site_hist):
        raise ValueError("--site-mixture fits the per-site histograms of the run: it needs --site-summary FILE and "
                         "--site-histogram BINS[:LO:HI]")
    if site_mixture and not 1 <= site_mixture <= 1024:
        raise ValueError(f"--site-mixture {site_mixture}: MAX_ITERS must be 1 .. 1024")
    if site_capacity and not site_summary:
        raise ValueError("--site-capacity sizes the sparse per-site table: it needs --site-summary FILE")
    if site_capacity and not 1 <= site_capacity <= 4294967294:
        raise ValueError(f"--site-capacity {site_capacity}: ROWS must be 1 .. 4294967294")
    if site_model_out and not site_mixture:
        raise ValueError("--site-model-out saves the fitted per-site mixtures: it needs --site-mixture")
    if site_model and not site_summary:
        raise ValueError("--site-model scores every row against its position's model beside the per-site table: it needs --site-summary FILE")
    if site_merge_ranks and not site_summary:
        raise ValueError("--site-merge-ranks adds the ranks' per-site tables: it needs --site-summary FILE")
    if site_table_in and not site_summary:
        raise ValueError("--site-table-in adds a saved per-site table into the run's: it needs --site-summary FILE")
    LAST_RUN.pop("site_rows_dropped", None)
    LAST_RUN.pop("site_model_dropped", None)
    site_refs = None
    control_table = None
    loaded_model = None
    tables_in = []
    if site_summary:
        # refused before anything is started: what the per-site table cannot do yet, and a BAM that is not mapped
        from dynamont_amd.bam_io import bam_references
        from dynamont_amd.sites import DYN_SITE_NONE, contig_offsets
        if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 and not site_merge_ranks:
            raise ValueError("--site-summary runs in one process: merging the per-site tables of several ranks is not built yet "
                             "without --site-merge-ranks, which has every rank fill a table of its own and rank 0 add them")
        if host_preprocess or ZSTD_PARALLEL_FRAMES or not _native_bam(basecalls):
            raise ValueError("--site-summary needs the basecalls as a mapped .bam read by the native reader (not with "
                             "--host-preprocess, --parallel-zstd-frames or DYN_PY_BAM=1)")
        names, lengths = bam_references(basecalls)
        if not names:
            raise ValueError(f"--site-summary: the header of {basecalls} has no reference sequences (an unaligned BAM); map the reads first")
        site_refs = (names, contig_offsets(lengths))
        if int(site_refs[1][-1]) >= DYN_SITE_NONE or int(site_refs[1][-1]) == 0:
            raise ValueError(f"--site-summary: the references hold {int(site_refs[1][-1])} positions; the table takes 1 .. 4294967294")
        if site_model:
            # refused before anything is started: a model fitted over other references
            from dynamont_amd.segmentation.utils import load_site_model
            loaded_model = load_site_model(site_model, names, lengths)
        for path in site_table_in:
            # refused before anything is started: a saved table of other references, or whose histograms are not the run's
            from dynamont_amd.segmentation.utils import check_site_control, load_site_table
            tables_in.append((path, load_site_table(path)))
            check_site_control(tables_in[-1][1], path, names, lengths, site_hist, flag="--site-table-in")
        if site_control:
            # refused before anything is started: a control of other references, without histograms or of other bins
            from dynamont_amd.segmentation.utils import check_site_control, load_site_table
            control_table = load_site_table(site_control)
            check_site_control(control_table, site_control, names, lengths, site_hist)
            if 2 * int(site_refs[1][-1]) >= DYN_SITE_NONE:
                raise ValueError(f"--site-control: the run and the control take 2 x {int(site_refs[1][-1])} sites; the table takes up to 4294967294"
                                 + (" with --site-capacity too: the site ids are 32-bit" if site_capacity else ""))
    from dynamont_amd import parallel
    comm, local_rank = parallel.init_from_env()
    rank, world = (comm.rank, comm.world) if comm else (0, 1)
    if comm:
        device = local_rank
        if rank == 0:
            print(f"exchange: {comm.implementation}", file=sys.stderr, flush=True)
        LAST_RUN["exchange"] = comm.implementation
    # Every process owns a native sink (csv_sink.cpp). One process: it writes the output file. One process per GPU: every
    # rank formats AND compresses its own rows into a part of the frame (compression is the largest host cost of the
    # output: 11 core-seconds per 32 768 reads -- left to rank 0 it would cap the job at one GPU's speed); at the end the
    # parts' bytes are gathered to rank 0, which appends them to its own and closes the frame. --parallel-zstd-frames keeps
    # the Python listener (rank 0) and the per-round gather of the formatted rows.
    native = not ZSTD_PARALLEL_FRAMES
    q = queue_mod.Queue() if (rank == 0 and not native) else None
    writer = None
    if q is not None:
        header = CSV_HEADER_EVENTS if event_stats else CSV_HEADER
        if segment_scores:
            header = header[:-1] + CSV_COLUMNS_SCORES + b"\n"
        if border_confidence:
            header = header[:-1] + CSV_COLUMNS_BORDERS + b"\n"
        if posterior_samples:
            header = header[:-1] + CSV_COLUMNS_SAMPLES + b"\n"
        if border_interval:
            header = header[:-1] + CSV_COLUMNS_INTERVALS + b"\n"
        if soft_levels:
            header = header[:-1] + CSV_COLUMNS_SOFT + b"\n"
        writer = threading.Thread(target=listener, args=(q, outfile, header), daemon=True)
        writer.start()
    sink = None if native else (q if comm is None else _Collector())
    is_rna = "rna" in pore

    def ship():  # one collective round: everything collected since the last round goes to rank 0
        rows, errs = sink.drain()
        all_rows = parallel.gather_bytes(comm, rows)
        all_errs = parallel.gather_bytes(comm, errs)
        if rank == 0:
            for blob in all_rows:
                if blob:
                    q.put(blob)
            for blob in all_errs:
                for line in blob.decode().split("\n") if blob else []:
                    q.put(line)

    def write_summary(aligner):
        # --kmer-summary, with the pipeline dry: every rank's raw integer arrays travel to rank 0 (one more gather), which adds
        # them as Python ints and writes the file -- the same bytes for any number of ranks
        if not kmer_summary:
            return
        from dynamont_amd._dynamont import kmer_summary_from_limbs
        from dynamont_amd.segmentation.utils import merge_kmer_summaries, write_kmer_summary
        mine = aligner.kmer_summary()
        parts = [mine]
        if comm is not None:
            t = np.array([mine["totals"][k] for k in ("reads_ok", "segments", "samples", "skipped_segments")], dtype=np.uint64)
            blobs = parallel.gather_bytes(comm, b"".join(c.tobytes() for c in mine["limbs"]) + t.tobytes())
            if rank != 0:
                return
            parts = []
            for blob in blobs:
                words = np.frombuffer(blob, dtype=np.uint64)
                n = aligner.num_kmers
                parts.append(kmer_summary_from_limbs([words[f * n:(f + 1) * n] for f in range(6)], words[6 * n:6 * n + 4]))
        mean, stdev = aligner.model_table()
        write_kmer_summary(kmer_summary, merge_kmer_summaries(parts), model_path, mean, stdev, aligner.rna)
        print(f"k-mer summary written: {kmer_summary}", file=sys.stderr, flush=True)

    site_counts = [0, 0]  # --site-summary: reads handed to the aligner, reads of those left without ids

    def merge_rank_tables(aligner, num_sites):
        # --site-merge-ranks, with the pipeline dry. Every rank > 0 packs the covered sites of its run's half [0, N) on its GPU
        # (Aligner.site_table_pack: only they cross to the host). The records travel to rank 0 rank by rank, as _gather_parts sends
        # the parts of the frame: in every round ONE rank sends a piece of at most 64 MB, header included -- header [n, first,
        # totals[5]] u64, cells [n][7] u64, site [n] u32, level [n][bins + 2] u32, dwell [n][16] u32 -- and rank 0 adds it by key
        # (Aligner.site_summary_merge) before the next round: rank 0 never holds more than one piece. The totals ride on a rank's
        # first piece (a rank without a covered site sends that piece with n = 0: the merge then adds the totals alone). Integers,
        # so the table is the same bits whatever the number of ranks and the order. An exception on any rank ends the whole job
        # (parallel.abort_on_error around segment()'s body). Returns (rows the ranks' own tables dropped, RECORDS the merge found
        # no bucket for -- a record is one rank's sums for one position), the same on every rank.
        t_start = _time.perf_counter()
        B = (aligner._site_histogram[0] + 2) if aligner._site_histogram else 0
        record = 56 + 4 + 4 * (B + 16 if B else 0)
        per_chunk = max(1, ((64 << 20) - 56) // record)
        mine = aligner.site_table_pack(0, num_sites) if rank != 0 else None
        t_pack = _time.perf_counter() - t_start
        n_mine = int(mine["site"].size) if mine is not None else 0
        own_dropped = aligner.site_map()["rows_dropped"] if site_capacity else 0
        edges = aligner.site_histogram(0, 0)["edges"] if B and rank == 0 else None
        merge_dropped = n_records = 0
        for src in range(1, world):
            sent = 0
            while True:
                payload = b""
                if rank == src:
                    a, b = sent, min(sent + per_chunk, n_mine)
                    head = np.array([b - a, 1 if a == 0 else 0] + [int(mine["totals"][k]) for k in mine["totals"]], dtype=np.uint64)
                    parts = [head, np.stack([c[a:b] for c in mine["limbs"]], axis=1) if b > a else np.zeros((0, 7), dtype=np.uint64),
                             mine["site"][a:b].astype(np.uint32)]
                    if B:
                        parts += [mine["level"][a:b], mine["dwell"][a:b]]
                    payload = b"".join(np.ascontiguousarray(p).tobytes() for p in parts)
                    sent = b
                blobs = parallel.gather_bytes(comm, payload)
                if rank == 0 and blobs[src]:
                    blob = blobs[src]
                    head = np.frombuffer(blob, dtype=np.uint64, count=7)
                    n = int(head[0])
                    at = 56
                    cells = np.frombuffer(blob, dtype=np.uint64, count=7 * n, offset=at).reshape(n, 7)
                    at += 56 * n
                    packed = {"site": np.frombuffer(blob, dtype=np.uint32, count=n, offset=at), "limbs": [cells[:, f] for f in range(7)],
                              "totals": [int(v) for v in head[2:7]] if int(head[1]) else None}
                    at += 4 * n
                    if B:
                        packed["level"] = np.frombuffer(blob, dtype=np.uint32, count=B * n, offset=at).reshape(n, B)
                        at += 4 * B * n
                        packed["dwell"] = np.frombuffer(blob, dtype=np.uint32, count=16 * n, offset=at).reshape(n, 16)
                        packed["edges"] = edges
                    n_records += n
                    before = aligner.site_map()["sites_dropped"] if site_capacity else 0
                    try:
                        aligner.site_summary_merge(packed)
                    except MemoryError:  # (a full sparse table: the records without a bucket are counted, the others were added)
                        merge_dropped += aligner.site_map()["sites_dropped"] - before
                if not parallel.any_rank(comm, rank == src and sent < n_mine):
                    break
        counts = np.array(site_counts + [own_dropped], dtype=np.uint64)
        blobs = parallel.gather_bytes(comm, counts.tobytes())
        total = np.zeros(4, dtype=np.uint64)
        if rank == 0:
            for blob in blobs:
                total[:3] += np.frombuffer(blob, dtype=np.uint64, count=3)
            total[3] = merge_dropped
            site_counts[0], site_counts[1] = int(total[0]), int(total[1])
            print(f"site tables merged: {n_records} records of {world - 1} ranks ({n_records * record} bytes) in "
                  f"{_time.perf_counter() - t_start - t_pack:.3f} s (exchange and merge; a rank's own pack before it: {t_pack:.3f} s on rank 0's clock)",
                  file=sys.stderr, flush=True)
        dropped = parallel.broadcast_str(comm, "%d %d" % (int(total[2]), int(total[3]))).split()
        return int(dropped[0]), int(dropped[1])

    def write_sites(aligner):
        # --site-summary, with the pipeline dry: the sites with coverage, a window of the table at a time
        if not site_summary:
            return
        from dynamont_amd.segmentation.utils import SITE_QUANTILE_PROBS, write_site_summary
        num_sites = int(site_refs[1][-1])
        ranks_dropped = merge_dropped = 0
        if comm is not None:
            # --site-merge-ranks: every rank's covered sites, packed on its GPU, into rank 0's table by key; rank 0 writes
            ranks_dropped, merge_dropped = merge_rank_tables(aligner, num_sites)
            LAST_RUN["site_rows_dropped"] = ranks_dropped + merge_dropped  # (every rank: the job ends with one exit status)
            if rank != 0:
                return
        # --site-histogram: the three quantile columns, reduced on the GPU window by window beside the table's window
        quantiles = (lambda lo, hi: aligner.site_quantiles(SITE_QUANTILE_PROBS, lo, hi)) if site_hist else None
        control = None
        if control_table is not None:
            # --site-control: the control sits in [N, 2N); compared on the GPU window by window beside the table's window
            from dynamont_amd.segmentation.utils import site_control_columns
            control = lambda lo, hi, run: site_control_columns(aligner.site_compare(lo, hi, num_sites + lo), run,  # noqa: E731
                                                               aligner.site_summary(num_sites + lo, num_sites + hi))
        mixture = None
        if site_mixture:
            # --site-mixture: fitted on the GPU window by window beside the table's window; with a control, pooled with [N, 2N)
            from dynamont_amd.segmentation.utils import site_mixture_columns
            pooled = control_table is not None
            mixture = lambda lo, hi: site_mixture_columns(aligner.site_mixture(lo, hi, num_sites + lo if pooled else None,  # noqa: E731
                                                                               max_iters=site_mixture), pooled)
        # --site-capacity: only the 2^20-id windows that hold a key are gathered (a genome-wide id space has thousands of empty ones)
        windows = aligner.site_map_windows(20).tolist() if site_capacity else None
        written = write_site_summary(site_summary, aligner.site_summary, num_sites, *site_refs, quantiles=quantiles, control=control,
                                     mixture=mixture, windows=windows)
        if site_model_out:
            # --site-model-out: the run's fit again, window by window, its accepted rows kept; the file is sparse
            from dynamont_amd.bam_io import bam_references
            from dynamont_amd.segmentation.utils import SITE_MODEL_COLUMNS, save_site_model
            parts = {k: [] for k in SITE_MODEL_COLUMNS + ("site",)}
            step = 1 << 20
            spans = [(w0, min(w0 + step, num_sites)) for w0 in (range(0, num_sites, step) if windows is None else [w * step for w in sorted(windows)])
                     if w0 < num_sites]
            for w0, w1 in spans:
                fit = aligner.site_mixture(w0, w1, num_sites + w0 if control_table is not None else None, max_iters=site_mixture)
                keep = np.flatnonzero(np.isin(fit["status"], (0, 2)))
                parts["site"].append((keep + w0).astype(np.uint64))
                for k in SITE_MODEL_COLUMNS:
                    parts[k].append(fit[k][keep])
            cols = {k: (np.concatenate(v) if v else np.zeros(0, dtype=np.uint64 if k == "site" else np.float64)) for k, v in parts.items()}
            cols["num_sites"] = num_sites
            saved = save_site_model(site_model_out, cols, *bam_references(basecalls), histogram=aligner._site_histogram)
            print(f"site model written: {site_model_out}: {saved} positions with a fitted model", file=sys.stderr, flush=True)
        if site_table_out:
            from dynamont_amd.bam_io import bam_references
            from dynamont_amd.segmentation.utils import save_site_table
            saved = save_site_table(site_table_out, aligner, *bam_references(basecalls), lo=0, hi=num_sites, windows=windows)   # the run's half only
            print(f"site table written: {site_table_out}: {saved} sites with coverage", file=sys.stderr, flush=True)
        t = aligner.site_summary(0, 0)["totals"]
        sparse = ""
        if site_capacity:
            m = aligner.site_map()
            sparse = f"; sparse table: {m['n_keys']} of {m['capacity']} rows taken, rows_dropped {m['rows_dropped']}"
            if comm is not None:  # the ranks' dropped rows and the sites the merge found no bucket for, summed
                m["rows_dropped"] = ranks_dropped + merge_dropped
                sparse += f" (rows dropped on the ranks {ranks_dropped}, records dropped in the merge {merge_dropped})"
            LAST_RUN["site_rows_dropped"] = m["rows_dropped"]
        print(f"site summary written: {site_summary}: {written} sites with coverage; reads_ok {t['reads_ok']}, rows_added {t['rows_added']}, "
              f"samples_added {t['samples_added']}, rows_without_site {t['rows_without_site']}, rows_skipped {t['rows_skipped']}; "
              f"reads left without ids (unmapped, secondary / supplementary, reverse strand, CIGAR in a CG tag or not covering the read): "
              f"{site_counts[1]} of {site_counts[0]}{sparse}", file=sys.stderr, flush=True)
        if site_capacity and m["rows_dropped"]:
            print(f"site summary INCOMPLETE: {m['rows_dropped']} rows of positions that found no row in the full table of {m['capacity']} "
                  f"(rows_skipped counts them too) were dropped; every position in {site_summary} is complete, positions are missing. "
                  + (f"(Of that count {ranks_dropped} are rows the ranks' own tables dropped and {merge_dropped} are RECORDS -- one rank's sums "
                     f"for one position -- that found no row in rank 0's table in the merge.) " if comm is not None else "")
                  + ("(A position that one rank dropped and another rank kept holds the other ranks' rows only.) " if ranks_dropped else "") +
                  f"Run again with a larger --site-capacity (exit status 3)", file=sys.stderr, flush=True)

    def write_band_report(lines):
        # --band-report, with the pipeline dry: every rank's lines travel to rank 0 (one more gather), which sorts and writes
        # them -- the same bytes for any number of ranks
        if not band_report:
            return
        if comm is not None:
            blobs = parallel.gather_bytes(comm, "\n".join(lines).encode())
            if rank != 0:
                return
            lines = [ln for blob in blobs if blob for ln in blob.decode().split("\n")]
        with open(band_report, "wb") as f:
            f.write(band_report_bytes(lines))
        print(f"band report written: {band_report}", file=sys.stderr, flush=True)

    def guide_summary(counts, rescue=(0, 0, 0, 0, 0)):
        # --guide-auto / --guide-rescue: this process's reads (every rank reports its own)
        if guide_auto:
            print(f"Reads aligned inside their own guide: {counts[0]}; of those, reads whose guide did not converge within "
                  f"{guide_rounds} alignments: {counts[1] if guide_rounds != 1 else 0}", file=sys.stderr, flush=True)
        if guide_rescue:
            print(f"Reads flagged by their band margin (below {guide_rescue_margin}): {rescue[0]}; rescued inside their own guide: "
                  f"{rescue[1]}, of those not converged within {guide_rounds} alignments: {rescue[2] if guide_rounds != 1 else 0}; "
                  f"left as aligned for want of memory: {rescue[3]}, because the rescue failed: {rescue[4]}", file=sys.stderr, flush=True)

    # A failing rank ends the whole job (parallel.abort): a barrier in a `finally` would leave the other ranks in
    # their next collective until the process-group timeout.
    with parallel.abort_on_error(comm):
        pipe = None
        try:
            _stamp("segment(): creating the aligner")
            aligner = Aligner(model_path, pore, mode=mode, threads=1, band=band, device=device)
            _stamp("aligner ready (model parsed, device initialised, tables uploaded)")
            if mem_budget_gib:
                aligner.set_mem_budget(int(mem_budget_gib * (1 << 30)))
            aligner.set_strict(strict_ties)
            if event_stats:
                aligner.set_event_stats(True)
            if rescale_iters:
                aligner.set_rescale(rescale_iters)
            if segment_scores:
                aligner.set_segment_scores(segment_scores)
            if border_confidence:
                aligner.set_border_confidence(border_confidence)
            if posterior_samples:
                aligner.set_posterior_samples(posterior_samples, sample_seed)
            if border_interval:
                aligner.set_border_interval(border_interval)
            if soft_levels:
                aligner.set_soft_levels(True)
            if kmer_summary:
                aligner.set_kmer_summary(True)
            if site_summary:
                try:
                    aligner.set_site_summary(int(site_refs[1][-1]) * (2 if control_table is not None else 1),  # --site-control: [N, 2N)
                                             capacity=site_capacity or None)
                except MemoryError as error:
                    if site_capacity:
                        raise MemoryError(f"--site-capacity: the sparse table of {site_capacity} rows (60 bytes each) does not fit: {error}") from None
                    raise MemoryError(f"--site-summary: the table of {int(site_refs[1][-1])} sites (56 bytes each) does not fit: {error}") from None
                if site_hist:
                    from dynamont_amd.segmentation.utils import site_histogram_range
                    bins, h_lo, h_hi = site_hist
                    if h_lo is None:
                        h_lo, h_hi = site_histogram_range(*aligner.model_table())
                    try:
                        aligner.set_site_histogram(bins, h_lo, h_hi)
                    except MemoryError as error:
                        if site_capacity:
                            raise MemoryError(f"--site-histogram: the counters of {site_capacity} rows ({4 * (bins + 18)} bytes each) "
                                              f"do not fit: {error}") from None
                        raise MemoryError(f"--site-histogram: the counters of {int(site_refs[1][-1])} sites ({4 * (bins + 18)} bytes each) "
                                          f"do not fit: {error}") from None
                    print(f"site histogram: {bins} bins over [{h_lo!r}, {h_hi!r})", file=sys.stderr, flush=True)
                    for path, table in tables_in:  # (a range left to the model table is known only now)
                        from dynamont_amd.segmentation.utils import check_site_control
                        check_site_control(table, path, site_refs[0], table["ref_lengths"], (bins, h_lo, h_hi), flag="--site-table-in")
                    if control_table is not None and rank == 0:  # (--site-merge-ranks: rank 0 writes; a control is counted once)
                        # before the first batch: the control into [N, 2N). (A range left to the model table is known only now.)
                        from dynamont_amd.segmentation.utils import check_site_control, load_site_control
                        check_site_control(control_table, site_control, site_refs[0], control_table["ref_lengths"], (bins, h_lo, h_hi))
                        try:
                            added = load_site_control(aligner, control_table, int(site_refs[1][-1]))
                        except MemoryError as error:
                            if not site_capacity:
                                raise
                            # a control that is only partly in the table would be compared as if it were whole: the run ends here,
                            # before any read is aligned and before the TSV exists
                            raise MemoryError(f"--site-capacity {site_capacity}: the control {site_control} does not fit the sparse table "
                                              f"beside the run ({error}); run again with a larger --site-capacity") from None
                        print(f"site control: {site_control}: {added} sites with coverage loaded", file=sys.stderr, flush=True)
            for path, table in tables_in if rank == 0 else []:
                # --site-table-in: into the run's half before the first batch, by key, totals included; on rank 0 only -- a saved
                # table is counted once
                from dynamont_amd.segmentation.utils import merge_site_table
                try:
                    added = merge_site_table(aligner, table, 0, totals=True)
                except MemoryError as error:
                    # a table that is only partly in would be reported as if it were whole: the run ends here
                    raise MemoryError(f"--site-capacity {site_capacity}: the table {path} does not fit the sparse table ({error}); "
                                      f"run again with a larger --site-capacity") from None
                print(f"site table in: {path}: {added} sites with coverage added", file=sys.stderr, flush=True)
            if loaded_model is not None:
                # --site-model: onto the GPU before the first ticket, beside the table; every ticket from here on is scored
                from dynamont_amd.segmentation.utils import upload_site_model
                try:
                    up = upload_site_model(aligner, loaded_model)
                except MemoryError as error:
                    raise MemoryError(f"--site-model: the model of {site_capacity or int(site_refs[1][-1])} rows (40 bytes each) does not fit: {error}") from None
                aligner.set_site_calls(True)
                LAST_RUN["site_model_dropped"] = up["dropped"]
                print(f"site model: {site_model}: {up['stored']} positions loaded" +
                      (f"; {up['dropped']} of them found no row in the sparse table of {site_capacity} rows and were dropped: their rows have no call"
                       if up["dropped"] else ""), file=sys.stderr, flush=True)
            if band_report:
                aligner.set_band_margin(True)
            if guide_auto:
                aligner.set_auto_guide(guide_auto, guide_rounds)
            if guide_rescue:
                aligner.set_guide_rescue(guide_rescue_margin, guide_rescue, guide_rounds)
            if native:
                import tempfile
                part, part_err = outfile, None
                if rank != 0:  # a part of the frame, in local scratch space; its bytes travel to rank 0 at the end
                    fd, part = tempfile.mkstemp(prefix=f"dynamont_part{rank}_", suffix=".zst")
                    os.close(fd)
                    part_err = part + ".errors"
                    parallel.register_scratch(part, part_err)  # gone with the job however it ends (parallel.abort included)
                # ONE frame out of every rank's blocks: all of them must be compressed for the window rank 0's frame header
                # declares, i.e. at rank 0's effective level -- a per-process DYN_SINK_LEVEL must not differ between ranks
                if comm is not None:
                    zstd_level = int(parallel.broadcast_str(comm, str(int(os.environ.get("DYN_SINK_LEVEL", zstd_level)))))
                    os.environ.pop("DYN_SINK_LEVEL", None)
                local_world = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world)))
                threads = host_threads or max(2, min(16, available_cpus() // local_world - (4 if local_world == 1 else 2)))
                pipe = sink = _NativePipeline(aligner, part, raw=not host_preprocess, depth=depth, threads=threads,
                                              first=rank == 0, last=world == 1, errfile=part_err, level=zstd_level)
                _stamp("sink open")
                if not host_preprocess and _native_bam(basecalls):
                    # BAM basecalls: the jobs arrive as columns (this rank's share of them); raw files that can point at their
                    # compressed chunks (.pod5, VBZ) are served without a Python object per read, any other reader read by read
                    for jb in job_batches(basecalls, minq, batch_reads, is_rna, rank, world,
                                          site_offsets=site_refs[1] if site_summary else None, site_counts=site_counts):
                        prepared = prepare_job_columns(jb, data_path, sink.put)
                        if prepared is not None:
                            pipe.submit_columns(*prepared)
                            if pipe.submitted <= 2:
                                _stamp("batch %d submitted" % (pipe.submitted - 1))
                            continue
                        pending = []
                        for i, job in enumerate(jobs_from_columns(jb, data_path)):
                            try:
                                signal, read, cal = prepare_job_raw(job, is_rna, oriented=True)
                            except Exception as error:  # noqa: BLE001  (segment.py:178-187)
                                sink.put(f"error: worker, {error}\tN: {int(jb.bases[i])}\tRid: {job[6]}\tSid: {job[7]}")
                                continue
                            pending.append((signal, read, job, cal, int(jb.bases[i]), jb.site_ids[i] if site_summary else None))
                        pipe.submit(pending)
                else:
                    pending = []
                    for job in generate_jobs(data_path, basecalls, minq, rank, world):
                        try:
                            if host_preprocess:
                                signal, read = prepare_job(job, is_rna)
                                cal = None
                            else:
                                signal, read, cal = prepare_job_raw(job, is_rna)
                        except Exception as error:  # noqa: BLE001  (segment.py:178-187)
                            sink.put(f"error: worker, {error}\tN: {len(job[5])}\tRid: {job[6]}\tSid: {job[7]}")
                            continue
                        pending.append((signal, read, job, cal))
                        if len(pending) >= batch_reads:
                            pipe.submit(pending)
                            pending = []
                    if pending:
                        pipe.submit(pending)
                _stamp("every batch submitted")
                pipe.close()
                guide_summary(pipe.guide_counts, pipe.rescue_counts)
                band_lines, pipe = pipe.band_lines, None
                _stamp("pipeline closed: output complete")
                if comm is not None:
                    _gather_parts(comm, parallel, outfile, part, part_err)
                write_summary(aligner)
                write_sites(aligner)
                write_band_report(band_lines)
                parallel.remove_scratch()
                print("Done with segmentation.", file=sys.stderr, flush=True)
                return
            pipe = _Pipeline(aligner, sink, raw=not host_preprocess, depth=depth)
            job_iter = generate_jobs(data_path, basecalls, minq, rank, world)
            exhausted = False
            rounds = 0
            while True:
                pending = []
                while len(pending) < batch_reads:
                    job = next(job_iter, None)
                    if job is None:
                        exhausted = True
                        break
                    try:
                        if host_preprocess:
                            signal, read = prepare_job(job, is_rna)
                            cal = None
                        else:
                            signal, read, cal = prepare_job_raw(job, is_rna)
                    except Exception as error:  # noqa: BLE001  (segment.py:178-187)
                        _, _, _, _, _, read, readid, signalid = job
                        sink.put(f"error: worker, {error}\tN: {len(read)}\tRid: {readid}\tSid: {signalid}")
                        continue
                    pending.append((signal, read, job, cal))
                pipe.submit(pending, end_of_round=comm is not None)
                if comm is None:
                    if exhausted:
                        break
                    continue
                # multi-rank: round k is on the GPU while round k-1 (complete on every rank) is shipped. Every rank
                # takes part in every round, with empty payloads once it has run out of reads.
                if rounds >= 1:
                    pipe.wait_round()
                    ship()
                rounds += 1
                if not parallel.any_rank(comm, not exhausted):
                    pipe.wait_round()
                    ship()
                    break
            pipe.close()
            guide_summary(pipe.guide_counts, pipe.rescue_counts)
            band_lines, pipe = pipe.band_lines, None
            write_summary(aligner)
            write_band_report(band_lines)
            print("Done with segmentation.", file=sys.stderr, flush=True)
        finally:
            if pipe is not None:  # an exception is on its way: release what is queued, keep the first error
                try:
                    pipe.close()
                except BaseException:  # noqa: BLE001
                    pass
            if q is not None:
                q.put("kill")
                writer.join()
            close_raw_cache()
    if comm is not None:
        comm.close()  # (collective: every rank has finished its exchanges)
    if comm is not None and comm.dist.is_initialized():
        comm.dist.barrier()  # normal completion only


def main(argv=None) -> None:
    _stamp("main() entered (interpreter started, modules imported)")
    args = parse(argv)
    outfile = args.outfile
    if isdir(outfile):
        outfile = join(outfile, "dynamont.csv.zst")
    elif not outfile.endswith(".zst"):
        outfile += ".zst"
    parent = dirname(outfile)
    if parent and not exists(parent):
        makedirs(parent, exist_ok=True)
    if args.model_path:
        model_path = args.model_path
        assert exists(model_path), "Model path does not exist"
    else:
        model_path = get_model(args.pore)
        assert exists(model_path), f"Default model not found for pore: {args.pore}, {model_path}"
    print(f"Loaded model: {basename(model_path)}", file=sys.stderr)
    global ZSTD_PARALLEL_FRAMES
    ZSTD_PARALLEL_FRAMES = bool(args.parallel_zstd_frames)
    segment(args.raw, args.basecalls, args.processes, outfile, model_path, args.pore, args.mode, args.qscore,
            device=args.device, batch_reads=args.batch_reads, mem_budget_gib=args.mem_budget,
            host_preprocess=args.host_preprocess, depth=args.depth, strict_ties=args.strict_ties, host_threads=args.host_threads,
            zstd_level=args.zstd_level, event_stats=args.event_stats, rescale_iters=args.rescale_iters,
            kmer_summary=args.kmer_summary, segment_scores=args.segment_scores,
            border_confidence=args.border_confidence, band_report=args.band_report, band=args.band,
            guide_auto=args.guide_auto, guide_rounds=args.guide_rounds, guide_rescue=args.guide_rescue,
            guide_rescue_margin=args.guide_rescue_margin, posterior_samples=args.posterior_samples, sample_seed=args.sample_seed,
            border_interval=args.border_interval, soft_levels=args.soft_levels, site_summary=args.site_summary, site_table_out=args.site_table_out,
            site_control=args.site_control, site_mixture=args.site_mixture,
            site_histogram=args.site_histogram, site_capacity=args.site_capacity, site_model_out=args.site_model_out,
            site_model=args.site_model, site_merge_ranks=args.site_merge_ranks, site_table_in=tuple(args.site_table_in))
    _stamp("segment() returned (aligner closed)")
    # --site-capacity: rows were dropped from a full table -- everything is written, the status says that sites are missing
    status = 3 if LAST_RUN.get("site_rows_dropped") else 0
    if argv is None and not int(__import__("os").environ.get("WORLD_SIZE", "1") or 1) > 1:
        # Invoked as the command (console script / python -m), single process, everything written and closed: leave without
        # the interpreter's and the HIP runtime's orderly teardown (0.3 s in which ~130 GB of device memory are handed back
        # allocation by allocation -- the driver reclaims them with the process anyway). Callers of main([...]) are not affected.
        import os
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(status)
    if status:
        sys.exit(status)


if __name__ == "__main__":
    main()
