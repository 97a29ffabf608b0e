"""The families of golden fixture G15 (test infrastructure): reads as real data has them -- basecalls that disagree with the
signal, heavy-tailed dwell with stalls, signal that hugs or leaves the band, fits nothing or lies far outside every density --
and tables whose neighbouring k-mers lie 1e-6 .. 1e-16 apart. Inputs are regenerated from seeds by everyone who needs them
(tests/golden/make_golden_g15.py, tests/test_imperfect_reads.py, tests/test_gpu_imperfect_reads.py, the campaign scripts);
the fixture holds the compiled reference's answers only.

A family is (pore, table, band, reads): ``FAMILIES[name]`` -> ``Family``; ``reads_of(name, tables)`` regenerates its reads.
"""
from __future__ import annotations

import os
import sys
import zlib
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from dynamont_amd import synth  # noqa: E402

PORES = ("rna002", "rna004", "dna_r9", "dna_r10_400bps")
ERROR_RATES = ((0.02, 0.01), (0.05, 0.03), (0.10, 0.06))   # (substitutions, insertions + deletions)
N_READS = 16          # per imperfect family
N_NEAR = 120          # per near-duplicate table
BASES = (100, 400)
EDGE_2E5 = 8          # which read of an edge family carries the 2e5 sample (at a quarter of the read)
WIDE_BASES = (470, 700)   # band 600: half band = min(300, columns / 2) > 223, the generic wide-band kernel

# tables: name -> (k, how to make it). "syn5" / "syn9" are the suite's models (conftest.models)
TABLES = {
    "syn5": (5, lambda: synth.model_values(5, 7, 0.25)),
    "syn9": (9, lambda: synth.model_values(9, 7, 0.15)),
    # near-duplicate tables: gaps of 1e-6 .. 1e-11 and 1e-12 .. 1e-16 in the mean, 1e-9 .. 1e-15 in the stdev
    "near5_mean_6_11": (5, lambda: synth.near_duplicate_table(5, range(6, 12), 1501, "mean", 0.25)),
    "near5_mean_12_16": (5, lambda: synth.near_duplicate_table(5, range(12, 17), 1502, "mean", 0.25)),
    "near5_stdev_9_15": (5, lambda: synth.near_duplicate_table(5, range(9, 16), 1503, "stdev", 0.25)),
    "near9_mean_6_11": (9, lambda: synth.near_duplicate_table(9, range(6, 12), 1504, "mean", 0.15)),
    "near9_mean_12_16": (9, lambda: synth.near_duplicate_table(9, range(12, 17), 1505, "mean", 0.15)),
    "near9_stdev_9_15": (9, lambda: synth.near_duplicate_table(9, range(9, 16), 1506, "stdev", 0.15)),
}


def table_for(pore: str) -> str:
    return "syn5" if synth.PORES[pore][2] == 5 else "syn9"


def write_tables(outdir: str, names=None) -> dict:
    """name -> (model path, mean, stdev as the aligner reads them back, file order)"""
    out = {}
    for name in (names or TABLES):
        k, make = TABLES[name]
        path = os.path.join(outdir, name + ".model")
        if not os.path.exists(path):
            synth.write_model_values(path, k, *make())
        _, mean, sd = synth.read_model_file(path)
        out[name] = (path, mean, sd)
    return out


@dataclass(frozen=True)
class Family:
    name: str
    pore: str
    table: str
    band: int
    kind: str          # "errors", "variant", "edge", "cfg2", "near", "found"
    arg: tuple
    n_reads: int
    noisy: bool = False   # far-out samples: the reference's own posteriors are coarse (|Z| huge)

    @property
    def seed(self) -> int:
        return zlib.crc32(self.name.encode()) & 0x7fffffff


def _errors(fam: Family, mean, sd):
    _, rna, k = synth.PORES[fam.pore]
    heavy, p_sub, p_indel, bases = fam.arg
    mean_c, sd_c = synth.code_order_table(mean, sd, k, rna)
    rng = np.random.default_rng(fam.seed)
    return [synth.imperfect_read(rng, mean_c, sd_c, k, int(rng.integers(bases[0], bases[1] + 1)), heavy, p_sub, p_indel, rna)
            for _ in range(fam.n_reads)]


_VARIANTS = {}


def _variant(fam: Family, mean, sd):
    """the seven stress variants of ONE set of base reads per pore; family v takes every 7th. A family renamed NAME#SEED (the
    campaigns) draws fresh base reads for that suffix."""
    suffix = fam.name.partition("#")[2]
    key = (fam.pore, fam.table, fam.n_reads, suffix)
    if key not in _VARIANTS:
        seed = zlib.crc32((f"variants_{fam.pore}" + ("#" + suffix if suffix else "")).encode()) & 0x7fffffff
        base = synth.make_reads(seed, fam.n_reads, fam.pore, mean, sd, BASES)
        _VARIANTS[key] = synth.stress_variants(base, np.random.default_rng(seed + 1), float(np.median(sd)))
    return _VARIANTS[key][synth.STRESS_VARIANTS.index(fam.arg[0])::len(synth.STRESS_VARIANTS)]


def _edge(fam: Family, mean, sd):
    """test_train_sample_at_the_edge_of_double_precision's reads: one sample at 1e4 (7e4 model standard deviations out: log
    density -2e9); read EDGE_2E5 of the family carries 2e5 instead (1e6 out, -9e11: the reference's two roundings of Z differ
    by more than its threshold there and it refuses the read on most pores -- one read, so that the family stays within the
    fixture's cap of 10 % refused reads)"""
    base = synth.make_reads(fam.seed, fam.n_reads, fam.pore, mean, sd, BASES)
    out = []
    for j, r in enumerate(base):
        s = r.signal.copy()
        s[len(s) // (j % 3 + 2)] = 2e5 if j == EDGE_2E5 else 1e4
        out.append(synth.SynthRead(s, r.sequence))
    return out


def _near(fam: Family, mean, sd):
    """short reads (many decisions per sample close to a near-duplicate pair), behind the pad one non-A base so that the
    pad itself ties nothing"""
    _, rna, k = synth.PORES[fam.pore]
    mean_c, sd_c = synth.code_order_table(mean, sd, k, rna)
    rng = np.random.default_rng(fam.seed)
    out = []
    for _ in range(fam.n_reads):
        digits = rng.integers(0, 4, size=int(rng.integers(fam.arg[0], fam.arg[1] + 1)))
        if rna:
            digits[:9] = 0
            digits[9] = int(rng.integers(1, 4))
        out.append(synth.read_from_digits(rng, digits, mean_c, sd_c, k, float(rng.choice([3.5, 10.0]))))
    return out


def _found(fam: Family, mean, sd):
    """the reads FOUND names, out of the campaign's 840 of their source family"""
    src, n, picks = fam.arg
    import dataclasses
    reads = _near(dataclasses.replace(FAMILIES[src], name=f"{src}#1", n_reads=n), mean, sd)
    return [reads[i] for i in picks]


_GEN = {"errors": _errors, "variant": _variant, "edge": _edge, "cfg2": _errors, "near": _near, "found": _found}


# what the campaign over 840 fresh reads per near-duplicate table found (tests/decision_margin.py --family near --reads 840
# --seed 1 --replay; profiles/imperfect/): source family -> read numbers. The first two: reads on which the plain arithmetic
# leaves the reference's borders although no neighbouring pair of columns has bit-equal parameters. The last two: reads with a
# margin below 1e-9 whose closest pair of columns is more than 1e-10 apart -- they decide the threshold's decade.
FOUND = {"rna004_near9_mean_12_16": (198, 709, 752), "rna004_near9_stdev_9_15": (310, 437, 504, 628, 722),
         "dna_r9_near5_mean_6_11": (756, 814), "rna004_near9_mean_6_11": (16, 154, 213, 310, 475, 640, 672, 703, 839)}
TIE_TAU = 1e-9        # dyn_tie_rows: neighbouring columns within this of each other in mean AND stdev count as a structural tie


def pair_gaps(kmers, mean_code, sd_code):
    """per neighbouring pair of columns: max(|d mean|, |d stdev|) (0 for equal k-mers); tables in k-mer-code order"""
    a, b = np.asarray(kmers[:-1]), np.asarray(kmers[1:])
    return np.maximum(np.abs(mean_code[a] - mean_code[b]), np.abs(sd_code[a] - sd_code[b]))


def _families():
    fams = []
    for pore in PORES:
        tb = table_for(pore)
        for heavy in (False, True):
            for p_sub, p_indel in ERROR_RATES:
                name = f"{pore}_{'heavy' if heavy else 'poisson'}_{round(100 * p_sub)}_{round(100 * p_indel)}"
                fams.append(Family(name, pore, tb, 400, "errors", (heavy, p_sub, p_indel, BASES), N_READS))
        for v in synth.STRESS_VARIANTS:
            fams.append(Family(f"{pore}_{v}", pore, tb, 400, "variant", (v,), N_READS, noisy=v == "far_out"))
        fams.append(Family(f"{pore}_edge", pore, tb, 400, "edge", (), N_READS, noisy=True))
        # band 50: the path leaves the band
        fams.append(Family(f"{pore}_squeezed_band50", pore, tb, 50, "variant", ("squeezed",), N_READS))
        fams.append(Family(f"{pore}_heavy_10_6_band50", pore, tb, 50, "errors", (True, 0.10, 0.06, BASES), N_READS))
    # cfg2-shaped: 2 000 bases, ~20 k samples -- paged sessions, certified prefixes
    fams.append(Family("rna004_cfg2_heavy_5_3", "rna004", "syn9", 400, "cfg2", (True, 0.05, 0.03, (2000, 2000)), 32))
    # band 600 on reads of more than 446 columns: the generic wide-band kernel
    for pore in ("rna004", "dna_r9"):
        fams.append(Family(f"{pore}_heavy_5_3_band600", pore, table_for(pore), 600, "errors", (True, 0.05, 0.03, WIDE_BASES), N_READS))
    for pore, k in (("dna_r9", 5), ("rna004", 9)):
        for tb in (f"near{k}_mean_6_11", f"near{k}_mean_12_16", f"near{k}_stdev_9_15"):
            fams.append(Family(f"{pore}_{tb}", pore, tb, 400, "near", (60, 160), N_NEAR))
    for src, picks in FOUND.items():
        pore, table = src.split("_near")[0], "near" + src.split("_near")[1]
        fams.append(Family(f"{src}_found", pore, table, 400, "found", (src, 840, picks), len(picks)))
    return {f.name: f for f in fams}


FAMILIES = _families()
NEAR_FAMILIES = tuple(n for n, f in FAMILIES.items() if f.kind == "near")
FOUND_FAMILIES = tuple(n for n, f in FAMILIES.items() if f.kind == "found")
IMPERFECT_FAMILIES = tuple(n for n, f in FAMILIES.items() if f.kind not in ("near", "found"))


def reads_of(name: str, tables: dict):
    fam = FAMILIES[name]
    _, mean, sd = tables[fam.table]
    return _GEN[fam.kind](fam, np.asarray(mean), np.asarray(sd))


def signal_crc(read) -> int:
    return zlib.crc32(np.ascontiguousarray(read.signal, dtype=np.float64).tobytes())


RANDOM_KINDS = tuple(f"{d}_{round(100 * s)}_{round(100 * i)}" for d in ("poisson", "heavy") for s, i in ERROR_RATES) + synth.STRESS_VARIANTS + ("edge",)


def random_read(rng: np.random.Generator, pore: str, mean, sd, near: bool = False):
    """One read of a family drawn at random (the campaign tests/fuzz_parity.py --imperfect): -> (read, family, noisy). ``near``: the table is a near-duplicate one -- half the reads are the fixture's
    short plain reads, half carry basecalling errors."""
    _, rna, k = synth.PORES[pore]
    mean_c, sd_c = synth.code_order_table(mean, sd, k, rna)
    kind = RANDOM_KINDS[int(rng.integers(0, 6 if near else len(RANDOM_KINDS)))]
    if near and rng.random() < 0.5:
        digits = rng.integers(0, 4, size=int(rng.integers(60, 161)))
        if rna:
            digits[:9] = 0
            digits[9] = int(rng.integers(1, 4))
        return synth.read_from_digits(rng, digits, mean_c, sd_c, k, float(rng.choice([3.5, 10.0]))), "near_plain", False
    nb = int(rng.integers(BASES[0], BASES[1] + 1))
    if kind in synth.STRESS_VARIANTS or kind == "edge":
        base = synth.make_read(rng, mean_c, sd_c, k, nb, 10.0 if rna else 12.5, rna)
        if kind == "edge":
            s = base.signal.copy()
            s[len(s) // int(rng.integers(2, 5))] = 2e5 if rng.random() < 0.1 else 1e4
            return synth.SynthRead(s, base.sequence), kind, True
        return synth.stress_variants([base], rng, float(np.median(sd)))[synth.STRESS_VARIANTS.index(kind)], kind, kind == "far_out"
    dwell, p_sub, p_indel = kind.split("_")
    return synth.imperfect_read(rng, mean_c, sd_c, k, nb, dwell == "heavy", int(p_sub) / 100, int(p_indel) / 100, rna), kind, False
