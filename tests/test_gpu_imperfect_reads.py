"""GPU (-m gpu): align() on imperfect reads and near-duplicate tables against golden fixture G15 (tests/golden/
g15_imperfect_reads.npz: the COMPILED REFERENCE's answers; families in tests/imperfect_families.py; CPU half and the fixture's
own checks in tests/test_imperfect_reads.py).

Every handle is used as created, in the default strict mode "ties". Per read: status and message are the reference's; segment
borders, base positions and the all-M states equal the fixture bit for bit; Z within 1e-9 relative, bit-identical wherever the
tie rule flags the read; posteriors against the live oracle within 1e-6 (on reads with far-out samples the reference's own
posteriors are only good to 1024 eps |Z|: the train tests' noise rule); the Z-only call answers with the same status and Z.
Then the same reads through every other device path -- one launch per batch (DYN_NO_SESSION=1), the in-place posterior layout,
a page-starved pool, asynchronous tickets with the families interleaved, band 50, band 600 (the generic wide-band kernel) --
each bit-equal to the default run and to the fixture. No tolerance on an integer column anywhere."""
import json
import multiprocessing as mp
import os

import numpy as np
import pytest

from conftest import golden
from dynamont_amd import Aligner, synth
from oracle import pyoracle
import imperfect_families as F

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]


@pytest.fixture(scope="module")
def g15(tmp_path_factory, oracle_built):
    g = golden("g15_imperfect_reads.npz")
    assert json.loads(str(g["families"])) == list(F.FAMILIES)
    tables = F.write_tables(str(tmp_path_factory.mktemp("g15models")))
    fams = {}
    for name, fam in F.FAMILIES.items():
        reads = F.reads_of(name, tables)
        assert np.array_equal(np.array([F.signal_crc(r) for r in reads], dtype=np.uint32), g[name + "_crc"]), f"{name}: regenerated inputs differ"
        fams[name] = dict(fam=fam, model=tables[fam.table][0], reads=reads)
    return g, fams


_ORC = {}


def _orc_init(model, pore_id, band):
    _ORC["o"] = pyoracle.Oracle(model, pore_id, band)


def _orc_prob(job):
    try:
        return _ORC["o"].align(job[0], job[1], True)["probabilities"]
    except RuntimeError as e:
        return str(e)


def oracle_probabilities(f):
    """the live oracle's posteriors (the fixture stores none), in a fork pool of at most 16 workers"""
    fam = f["fam"]
    with mp.get_context("fork").Pool(min(16, os.cpu_count() or 1), initializer=_orc_init,
                                     initargs=(f["model"], synth.PORES[fam.pore][0], fam.band)) as pool:
        return pool.map(_orc_prob, [(r.signal, r.sequence) for r in f["reads"]], chunksize=1)


def check_read(g, name, i, res, j, z_bits=False):
    """read i of family `name` == result row j: the fixture's status / message / borders / base positions / states, Z within
    1e-9 relative and bit-identical where the rule flags the read (or everywhere: z_bits). Returns 1 for an integer mismatch
    -- counted by the caller, asserted at the end so that a failure names every read."""
    where = (name, i)
    if g[name + "_status"][i]:
        assert res.status[j] != 0 and res.error(j) == str(g[name + "_message"][i]), (where, int(res.status[j]), res.error(j))
        return 0
    assert res.status[j] == 0, (where, res.error(j))
    a, b = int(g[name + "_seg_off"][i]), int(g[name + "_seg_off"][i + 1])
    ra = int(res.seg_offsets[j])
    rb = ra + int(res.n_segments[j])
    same = (rb - ra == b - a and np.array_equal(res.signal_positions[ra:rb], g[name + "_sigpos"][a:b].astype(np.uint64))
            and np.array_equal(res.sequence_positions[ra:rb], g[name + "_seqpos"][a:b].astype(np.uint64))
            and bool((res.states[ra:rb] == ord("M")).all()) == bool(g[name + "_all_M"][i]))
    Z, want = float(res.Z[j]), float(g[name + "_Z"][i])
    if z_bits or g[name + "_rows"][i]:
        assert Z == want, (where, Z, want)
    else:
        assert abs(Z - want) <= 1e-9 * max(1.0, abs(want)), (where, Z, want)
    return 0 if same else 1


def same_answers(a, ja, b, jb):
    """two result rows bit-equal in status, Z and every integer column"""
    if a.status[ja] != b.status[jb] or (a.status[ja] == 0 and a.Z[ja] != b.Z[jb]) or a.n_segments[ja] != b.n_segments[jb]:
        return False
    sa, sb, n = int(a.seg_offsets[ja]), int(b.seg_offsets[jb]), int(a.n_segments[ja])
    return (np.array_equal(a.signal_positions[sa:sa + n], b.signal_positions[sb:sb + n])
            and np.array_equal(a.sequence_positions[sa:sa + n], b.sequence_positions[sb:sb + n])
            and np.array_equal(a.states[sa:sa + n], b.states[sb:sb + n]))


@pytest.mark.parametrize("name", list(F.FAMILIES))
def test_default_handle_equals_the_reference(g15, name):
    """pore x family, handle as created (band 50 / 600 families under their band; 600 = the generic wide-band kernel, whose Z is
    the reference's bit for bit on every read, the Z-only call included)"""
    g, fams = g15
    f = fams[name]
    fam, reads = f["fam"], f["reads"]
    sigs, seqs = [r.signal for r in reads], [r.sequence for r in reads]
    wide = fam.band == 600
    al = Aligner(f["model"], fam.pore, band=fam.band, device=0)
    with al.batch(sigs, seqs) as b:
        b.align(True)
        res = b.fetch()
        n_strict = b.timing()["reads_strict"]
    zonly = al.align_batch(sigs, seqs, False)
    al.close()
    rows = g[name + "_rows"]
    if not wide:
        assert n_strict == int((rows != 0).sum()), (name, n_strict)    # the rule flags exactly the reads dyn_tie_rows names
    want_p = oracle_probabilities(f)
    mismatches, worst_p, worst_z = [], 0.0, 0.0
    for i in range(len(reads)):
        mismatches += [i] * check_read(g, name, i, res, i, z_bits=wide)
        assert zonly.status[i] == res.status[i] and zonly.n_segments[i] == 0, (name, i, zonly.error(i))
        if res.status[i] != 0:
            assert want_p[i] == res.error(i), (name, i)
            continue
        want_z = float(g[name + "_Z"][i])
        if wide:
            assert zonly.Z[i] == want_z, (name, i)
        else:
            assert abs(zonly.Z[i] - want_z) <= 1e-9 * max(1.0, abs(want_z)), (name, i, zonly.Z[i], want_z)
        worst_z = max(worst_z, abs(res.Z[i] - want_z) / max(1.0, abs(want_z)))
        if i in mismatches:
            continue
        a = int(res.seg_offsets[i])
        dp = float(np.abs(res.probabilities[a:a + int(res.n_segments[i])] - want_p[i]).max())
        bound = max(1e-6, 1024 * 2.2e-16 * abs(want_z)) if fam.noisy else 1e-6
        worst_p = max(worst_p, dp / bound)
        assert dp <= bound, (name, i, dp, bound, want_z)
    print(f"G15 {name}: {len(reads)} reads, {int(g[name + '_status'].sum())} refused, {n_strict} flagged, integer mismatches {mismatches}, "
          f"max |dZ|/|Z| {worst_z:.1e}, max |dp| / bound {worst_p:.2e}")
    assert not mismatches, (name, mismatches)


def _band400_batches(fams, pore):
    """the band-400 families of a pore, grouped by table: [(model, [(family, read index, read), ...] interleaved)]"""
    by_table = {}
    for name, f in fams.items():
        if f["fam"].pore == pore and f["fam"].band == 400:
            by_table.setdefault(f["model"], []).append(name)
    out = []
    for model, names in by_table.items():
        items = []
        for i in range(max(len(fams[n]["reads"]) for n in names)):    # round robin: the families interleaved
            items += [(n, i, fams[n]["reads"][i]) for n in names if i < len(fams[n]["reads"])]
        out.append((model, items))
    return out


def _run(model, pore, items, budget=None):
    al = Aligner(model, pore, band=400, device=0)
    if budget:
        al.set_mem_budget(budget)
    with al.batch([r.signal for _, _, r in items], [r.sequence for _, _, r in items]) as b:
        b.align(True)
        res = b.fetch()
        tm = b.timing()
    tm["sessions"] = al.session_stats()["sessions"]
    al.close()
    return res, tm


@pytest.mark.parametrize("path", ["no_session", "inplace", "page_starved", "async"])
@pytest.mark.parametrize("pore", F.PORES)
def test_other_device_paths_equal_the_default_run_and_the_reference(g15, monkeypatch, pore, path):
    """All band-400 families of a pore (its near-duplicate tables included), interleaved in one batch per table, through: one
    launch per batch instead of the resident queue; the in-place posterior layout; a pool too small for the batch, so that
    reads queue for pages (RNA004: the 32 cfg2-shaped reads of ~20 k samples); asynchronous tickets, several in flight. Each is
    bit-equal to the default run of the same batch -- status, Z, every integer column -- and to G15."""
    g, fams = g15
    mismatches = []
    for model, items in _band400_batches(fams, pore):
        base, _ = _run(model, pore, items)
        if path == "no_session":
            monkeypatch.setenv("DYN_NO_SESSION", "1")
            res, tm = _run(model, pore, items)
            monkeypatch.delenv("DYN_NO_SESSION")
            assert tm["sessions"] == 0 and tm["launches"] >= 1, tm    # no resident queue: the handle launched per batch
        elif path == "inplace":
            monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
            res, tm = _run(model, pore, items)
            monkeypatch.delenv("DYN_FORCE_LAYOUT")
            assert tm["lp_inplace"] == 1
        elif path == "page_starved":
            # a read's lattice takes ~(448 * 8 + 56) bytes per row (tests/test_gpu_parity.py); room for a fifth of the batch,
            # and for the longest read one and a half times over
            lens = sorted((len(r.signal) for _, _, r in items), reverse=True)
            res, tm = _run(model, pore, items, budget=int(max(0.2 * sum(lens), 1.5 * lens[0]) * (448 * 8 + 56)))
            if any(n == "rna004_cfg2_heavy_5_3" for n, _, _ in items):
                assert 0 < tm["n_static"] < len(items), tm    # the cfg2-shaped reads queue for pages
        else:
            al = Aligner(model, pore, band=400, device=0)
            cuts = [0, len(items) // 5, len(items) // 2, len(items)]
            tickets = [al.align_async(*synth.pack_reads([r for _, _, r in items[a:b]]), True) for a, b in zip(cuts[:-1], cuts[1:])]
            parts = [t.wait() for t in tickets]
            for (a, b), part in zip(zip(cuts[:-1], cuts[1:]), parts):
                for j in range(b - a):
                    n, i, _ = items[a + j]
                    mismatches += [(n, i)] * check_read(g, n, i, part, j)
                    assert same_answers(part, j, base, a + j), (n, i)
            for t in tickets:
                t.close()
            al.close()
            continue
        for j, (n, i, _) in enumerate(items):
            mismatches += [(n, i)] * check_read(g, n, i, res, j)
            assert same_answers(res, j, base, j), (path, n, i)
    print(f"G15 {pore} via {path}: integer mismatches {mismatches}")
    assert not mismatches


def test_event_stats_and_rescale_off_leave_the_borders_alone(g15):
    """The opt-ins on the heavy-dwell 5/3 % family: set_event_stats(True) and set_rescale(0) change no border, no Z; the levels
    are the host definition's (tests/test_event_stats_host.py) bit for bit."""
    from test_event_stats_host import levels_of
    g, fams = g15
    name = "rna004_heavy_5_3"
    f = fams[name]
    sigs, seqs = [r.signal for r in f["reads"]], [r.sequence for r in f["reads"]]
    al = Aligner(f["model"], "rna004", device=0)
    base = al.align_batch(sigs, seqs, True)
    al.set_event_stats(True)
    al.set_rescale(0)
    on = al.align_batch(sigs, seqs, True)
    al.close()
    assert on.rescale_shift is None
    for i in range(len(sigs)):
        assert check_read(g, name, i, on, i) == 0 and same_answers(on, i, base, i), i
        a, b = int(on.seg_offsets[i]), int(on.seg_offsets[i]) + int(on.n_segments[i])
        want = levels_of(sigs[i], on.signal_positions[a:b])
        got = np.stack([on.level_mean[a:b], on.level_stdv[a:b], on.level_median[a:b]])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), i
