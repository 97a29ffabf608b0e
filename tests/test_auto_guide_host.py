"""CPU: the host half of the self-guided band (dyn_batch_auto_guide, dyn_batch_set_guide_refine). The g++ build of the pre-pass
(dynamont_amd/csrc/auto_guide_kernels.hpp) against its NumPy restatement, entry for entry; the purpose, shown on the CPU first:
the pre-pass guide and one alignment inside it give the borders of the full lattice on stalled reads, and refinement from the
plain diagonal reaches them too; every host-side refusal of the new entry points with its text, on a handle without a device."""
import os
import re

import numpy as np
import pytest

import auto_guide_cases as ac
import guided_band_cases as gc
from conftest import ROOT
from dynamont_amd import Aligner, _native as N, synth
from dynamont_amd.segmentation import train as train_cli
from oracle.pyoracle import Oracle

pytestmark = pytest.mark.usefixtures("native_lib")

HW = gc.STALL_HALF_WIDTH


@pytest.fixture(scope="module")
def ctx(models, tmp_path_factory):
    _, mean, sd = synth.read_model_file(models["syn5"])
    al = Aligner(models["syn5"], gc.PORE, device="host")
    assert al.info.log_e1 == 0.0
    c = dict(fam=gc.build_reads(mean, sd), m1=float(al.info.log_m1), e2=float(al.info.log_e2), model=models["syn5"],
             orc=Oracle(models["syn5"], synth.PORES[gc.PORE][0], 4093), host=ac.build_host(tmp_path_factory.mktemp("ag_host")),
             edge=ac.edge_reads(*synth.code_order_table(mean, sd, gc.K, False)))
    al.close()
    return c


def params(ctx, r):
    km = ctx["orc"].kmers(r.sequence)
    mean, sd = ctx["orc"].table()
    return np.ascontiguousarray(mean[km]), np.ascontiguousarray(sd[km]), -np.log(np.ascontiguousarray(sd[km]))


# ---- 1. the host build against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hw", [("stall", 16), ("stall_mv", 16), ("b", 16), ("a", 16), ("e", 16), ("e", 3), ("edge", 16), ("edge", 2)])
def test_host_build_equals_the_restatement(ctx, name, hw):
    reads = list(ctx["edge"].values()) if name == "edge" else ctx["fam"][name][:16] if name == "a" else ctx["fam"][name]
    if (name, hw) == ("e", 3):                                         # (every read of e at half width 16; a narrower window on 100)
        reads = reads[:100]
    assert len(reads) >= 3
    moved = 0
    for i, r in enumerate(reads):
        mean, sd, nls = params(ctx, r)
        want = ac.prepass_guide(r.signal, mean, sd, nls, ctx["m1"], ctx["e2"], hw)
        got = ac.host_guide(ctx["host"], r.signal, mean, sd, nls, ctx["m1"], ctx["e2"], hw)
        assert np.array_equal(got, want), (name, i, np.flatnonzero(got != want)[:5])
        assert ac.guide_invariants(got, r.n_kmers + 1) and got.max(initial=0) <= r.n_kmers, (name, i)
        moved += not np.array_equal(got, gc.diagonal(r))
    assert moved >= len(reads) // 2                                    # the guide is made from the signal, not the diagonal


def test_edge_reads_are_what_they_claim(ctx):
    e = ctx["edge"]
    assert e["n2"].n_kmers == 1 and len(e["tight"].signal) == 2 * e["tight"].n_kmers and np.isnan(e["nan"].signal).sum() == 1
    r = e["tight"]                                                     # lo == hi in every row: the guide is forced
    mean, sd, nls = params(ctx, r)
    g = ac.host_guide(ctx["host"], r.signal, mean, sd, nls, ctx["m1"], ctx["e2"], 4)
    assert g.tolist() == [(t + 1) // 2 for t in range(1, len(r.signal) + 1)]
    r = e["nan"]
    mean, sd, nls = params(ctx, r)
    g = ac.host_guide(ctx["host"], r.signal, mean, sd, nls, ctx["m1"], ctx["e2"], 8)
    assert ac.guide_invariants(g, r.n_kmers + 1)


# ---- 2. the purpose ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(ctx):
    """name -> the full lattice's borders of every read: model_align with a window of N columns"""
    out = {}
    for name in ("stall", "stall_mv", "b", "a"):
        reads = ctx["fam"][name][:16]
        out[name] = []
        for r in reads:
            mean, sd, _ = params(ctx, r)
            mo = gc.model_align(r.signal, mean, sd, ctx["m1"], ctx["e2"], gc.diagonal(r), r.n_kmers + 1)
            assert mo.ok
            out[name].append(mo.signal_positions)
    return out


@pytest.mark.parametrize("name", ["stall", "stall_mv", "b", "a"])
def test_prepass_and_one_alignment_find_the_full_lattices_borders(ctx, full, name):
    reads = ctx["fam"][name][:16]
    assert len(reads) == (6 if name == "stall_mv" else 16)
    for i, r in enumerate(reads):
        mean, sd, nls = params(ctx, r)
        g = ac.host_guide(ctx["host"], r.signal, mean, sd, nls, ctx["m1"], ctx["e2"], HW)
        mo = gc.model_align(r.signal, mean, sd, ctx["m1"], ctx["e2"], g, HW)
        assert mo.ok and np.array_equal(mo.signal_positions, full[name][i]), (name, i)


@pytest.mark.parametrize("name", ["stall", "stall_mv"])
def test_refinement_from_the_diagonal_reaches_them(ctx, full, name):
    seen = set()
    for i, r in enumerate(ctx["fam"][name]):
        mean, sd, _ = params(ctx, r)
        rounds, conv, g, mo, zs = ac.refine(r.signal, mean, sd, ctx["m1"], ctx["e2"], gc.diagonal(r), HW, 8)
        assert conv == 1 and rounds <= 8 and mo.ok, (name, i, rounds)
        assert np.array_equal(mo.signal_positions, full[name][i]), (name, i)
        assert all(b >= a for a, b in zip(zs, zs[1:])), (name, i, zs)     # Z never decreases
        assert np.array_equal(ac.next_guide(mo), g)
        seen.add(rounds)
    print("alignments until the fixed point, %s: %s" % (name, sorted(seen)))
    assert max(seen) >= 3                                              # the diagonal is not the answer: refinement does work


# ---- 3. refusals on a handle without a device ------------------------------------------------------------------------------
def test_symbols_header_and_abi(native_lib):
    hdr = open(os.path.join(ROOT, "include", "dynamont_mi.h")).read()
    assert re.search(r"#define DYN_ABI_VERSION 10\b", hdr)
    for decl in (r"int dyn_batch_auto_guide\(dyn_batch\* b, uint32_t half_width\);",
                 r"int dyn_batch_set_guide_refine\(dyn_batch\* b, uint32_t max_rounds\);",
                 r"int dyn_batch_fetch_guide\(dyn_batch\* b, int32_t\* out, uint64_t count\);",
                 r"int dyn_batch_fetch_guide_rounds\(dyn_batch\* b, uint32_t\* rounds, uint32_t\* converged, uint64_t n\);"):
        assert re.search(decl, hdr), decl
    for name in ("dyn_batch_auto_guide", "dyn_batch_set_guide_refine", "dyn_batch_fetch_guide", "dyn_batch_fetch_guide_rounds"):
        assert name in N.SIGNATURES and getattr(native_lib, name) is not None
    assert "auto_guide.hip" in N.SOURCES and "auto_guide_kernels.hpp" in N.HEADERS
    assert native_lib.dyn_batch_auto_guide(None, 8) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_batch_set_guide_refine(None, 2) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_batch_fetch_guide(None, None, 0) == N.DYN_ERR_INVALID_ARGUMENT
    assert native_lib.dyn_batch_fetch_guide_rounds(None, None, None, 0) == N.DYN_ERR_INVALID_ARGUMENT


def test_every_refusal_with_its_text(ctx):
    reads = ctx["fam"]["b"][:3]
    al = Aligner(ctx["model"], gc.PORE, band=50, device="host")
    flat = np.concatenate([gc.diagonal(r) for r in reads])
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        for hw in (0, 2047, 100000):
            with pytest.raises(ValueError, match=r"dyn_batch_auto_guide: half_width %d is outside \[1, 2046\]" % hw):
                b.auto_guide(hw)
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            b.auto_guide(16)
        with pytest.raises(ValueError, match="dyn_batch_set_guide_refine: the batch carries no guide"):
            b.set_guide_refine(4)
        with pytest.raises(ValueError, match="dyn_batch_fetch_guide: the batch carries no guide"):
            b.guide()
        with pytest.raises(ValueError, match="dyn_batch_fetch_guide_rounds: the batch carries no guide"):
            b.guide_rounds()
        b.set_guide(flat, 8)
        for rounds in (0, 65, 1000):
            with pytest.raises(ValueError, match=r"dyn_batch_set_guide_refine: max_rounds %d is outside \[1, 64\]" % rounds):
                b.set_guide_refine(rounds)
        with pytest.raises(ValueError, match="dyn_batch_fetch_guide_rounds: the batch was not aligned with calc_probabilities = 1"):
            b.guide_rounds()
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            b.guide()
        b.set_guide_refine(1)
        b.set_guide_refine(64)
        with pytest.raises(ValueError, match=r"dyn_batch_align: the batch refines its guide \(dyn_batch_set_guide_refine, max_rounds 64\)"):
            b.align(False)                                             # the Z-only job has no called path
        with pytest.raises(ValueError, match=r"dyn_batch_train_guided: the batch refines its guide"):
            b.train_guided()
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            b.align(True)
        b.set_guide_refine(1)                                          # back to today's behaviour: the refusals are gone
        with pytest.raises(RuntimeError, match="no GPU bound to this handle"):
            b.train_guided()
    al.close()


def test_cli_flags():
    base = ["-r", "x", "-b", "y", "-o", "z", "-p", "rna004", "--model_path", "m"]
    args = train_cli.parse(base)
    assert args.guide_auto == 0 and args.guide_rounds == 8
    args = train_cli.parse(base + ["--guide-auto", "16", "--guide-rounds", "4"])
    assert args.guide_auto == 16 and args.guide_rounds == 4
    with pytest.raises(SystemExit):
        train_cli.parse(base + ["--guide-auto", "16", "--guide-moves", "16"])
