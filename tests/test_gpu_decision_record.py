"""GPU (-m gpu): the forward sweep's per-row record as one byte per lane (dynamont_amd/csrc/decision_record.hpp) and the
sweeps' running row addresses (band_runs.hpp: fwd_run_end, bwd_run_first), end to end.

Every batch runs through the resident session and with sessions off (DYN_NO_SESSION=1), each time with a handle as created
and with one created under DYN_LPE_STORE_FLOOR=dense. The four results are equal bit for bit -- status, Z, every integer
column, every probability -- and one of them is compared with the CPU oracle: Z to 1e-9 relative, integer columns and status
equal, posteriors within 1e-6 (tests/test_gpu_parity.py's PROB_TIGHT).

Most batches run under DYN_PAGE_LOG_ROWS=2: lattice pages of the fewest rows the longest read allows (4 .. 32 for these
reads, 256 without the switch), so that a row cursor of either sweep crosses a page every few rows -- the case the running
addresses can get wrong. timing() must report page_rows <= 32 there."""
import numpy as np
import pytest

from conftest import model_for
from dynamont_amd import Aligner, synth
from oracle.pyoracle import Oracle
import test_gpu_sparse_posteriors as SP

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib", "oracle_built")]

PROB_TIGHT = SP.PROB_TIGHT
_ORACLE = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_parked_pool():
    """The tickets of 512 reads here open paged sessions whose lattice pool takes most of the card, and a closed handle parks
    its pool for its successor in this process: the larger pool stays parked. Later test files start child processes on the
    same card (tests/test_gpu_multirank_cli.py: bench.py with two ranks) that then find the memory taken. Give it back."""
    yield
    import dynamont_amd
    dynamont_amd.release_cached_memory()


def oracle_of(key, model, pore, reads, band=400):
    """Oracle.align(calc=True) of every read, computed once per batch: a dict, or the message of its refusal"""
    if key not in _ORACLE:
        orc = Oracle(model, synth.PORES[pore][0], band)
        out = []
        for r in reads:
            try:
                out.append(orc.align(r.signal, r.sequence, True))
            except RuntimeError as e:
                out.append(str(e))
        _ORACLE[key] = out
    return _ORACLE[key]


def check_oracle(res, wants, what):
    worst, refused = 0.0, 0
    for i, want in enumerate(wants):
        if isinstance(want, str):
            assert res.status[i] != 0 and res.error(i) == want, (what, i, res.error(i), want)
            refused += 1
            continue
        got = res.read(i)
        assert res.status[i] == 0, (what, i, res.error(i))
        assert np.array_equal(got["sequence_positions"], want["sequence_positions"]), (what, i)
        assert np.array_equal(got["signal_positions"], want["signal_positions"]), (what, i)
        assert got["states"] == want["states"], (what, i)
        assert abs(got["Z"] - want["Z"]) <= 1e-9 * max(1.0, abs(want["Z"])), (what, i)
        dp = float(np.abs(got["probabilities"] - want["probabilities"]).max())
        worst = max(worst, dp)
        assert dp <= PROB_TIGHT, (what, i, dp)
    print(f"{what}: {len(wants)} reads, {refused} refused by the oracle, max |dp| against the oracle {worst:.2e}")


def run(monkeypatch, model, pore, reads, floor, session, log_rows=None, budget=None):
    """one batch -> (result, timing). session: published into the resident read queue; else one launch per batch."""
    if log_rows is not None:
        monkeypatch.setenv("DYN_PAGE_LOG_ROWS", str(log_rows))
    if not session:
        monkeypatch.setenv("DYN_NO_SESSION", "1")
    try:
        al = SP.handle(monkeypatch, floor, model, pore)
        if budget:
            al.set_mem_budget(budget)
        if session and not budget:
            t = al.align_async(*synth.pack_reads(reads), True)
            res, tm = t.wait(), t.timing()
            assert tm["launches"] == 0, tm          # published into the resident session
            t.close()
        else:
            with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
                b.align(True)
                res, tm = b.fetch(), b.timing()
            if not session:
                assert al.session_stats()["sessions"] == 0 and tm["launches"] >= 1, tm
        al.close()
    finally:
        monkeypatch.delenv("DYN_PAGE_LOG_ROWS", raising=False)
        monkeypatch.delenv("DYN_NO_SESSION", raising=False)
    return res, tm


SESSION_MIN_READS = 512   # engine.hpp: a handle opens a session only for a ticket of at least this many reads


def four_way(monkeypatch, key, model, pore, reads, log_rows=2, filler=None):
    """session / no session x default / dense, bit for bit; the first against the oracle. Returns {(session, floor): timing}.
    The batch is the reads repeated until a ticket of them opens a session (the sweeps of 512 such reads take milliseconds);
    the oracle sees each read once. filler: other reads that fill the ticket instead (behind the reads; no oracle)."""
    first, tms = None, {}
    batch = reads + filler if filler else reads * -(-SESSION_MIN_READS // len(reads))
    assert len(batch) >= SESSION_MIN_READS
    for session in (True, False):
        for floor in (None, "dense"):
            res, tm = run(monkeypatch, model, pore, batch, floor, session, log_rows)
            tms[(session, floor)] = tm
            if first is None:
                first = res
                check_oracle(res, oracle_of(key, model, pore, reads), key)
            else:
                SP.assert_same_bits(first, res, (key, session, floor))
    print(f"{key}: page_rows {sorted({tm['page_rows'] for tm in tms.values()})}")
    return first, tms


def fit_length(read, n_samples):
    """the first n_samples samples of a read and the bases they cover (the same fraction of the sequence)"""
    assert len(read.signal) >= n_samples
    nb = max(12, int(len(read.sequence) * n_samples / len(read.signal)))
    return synth.SynthRead(np.ascontiguousarray(read.signal[:n_samples]), read.sequence[:nb])


def test_long_reads_wrap_the_slot_ring_on_small_pages(models, monkeypatch):
    """16 rna004 reads of 900-1 000 bases: N > 448 + 401, so the path and the band window wrap the slot ring and visit every
    (lane, cell) of the record; pages of at most 32 rows."""
    reads = SP.reads_for(models, "rna004", 7101, 16, (900, 1000))
    assert min(len(r.sequence) for r in reads) - 8 > 448 + 401
    first, tms = four_way(monkeypatch, "rna004 900-1000 bases", models["syn9"], "rna004", reads)
    assert (first.status == 0).all()
    assert all(tm["page_rows"] <= 32 for tm in tms.values()), {k: tm["page_rows"] for k, tm in tms.items()}


def test_short_reads_half_band_is_half_the_read(models, monkeypatch):
    """16 reads of 150-400 bases: bw = N / 2, most lanes of a row outside the band; pages of 4-16 rows"""
    reads = SP.reads_for(models, "rna004", 7102, 16, (150, 400))
    _, tms = four_way(monkeypatch, "rna004 150-400 bases", models["syn9"], "rna004", reads)
    assert all(tm["page_rows"] <= 32 for tm in tms.values())


def test_stress_variants(models, monkeypatch):
    _, mean, sd = synth.read_model_file(models["syn9"])
    base = synth.make_reads(7103, 3, "rna004", mean, sd, (150, 520))
    reads = synth.stress_variants(base, np.random.default_rng(7104), float(np.median(sd)))
    four_way(monkeypatch, "rna004 stress variants", models["syn9"], "rna004", reads)


def test_imperfect_reads(models, monkeypatch):
    """basecalls with substitutions and indels: diffuse posteriors, several stored lane groups per row"""
    _, mean, sd = synth.read_model_file(models["syn9"])
    _, rna, k = synth.PORES["rna004"]
    mean_code, sd_code = synth.code_order_table(mean, sd, k, rna)
    rng = np.random.default_rng(7105)
    reads = [synth.imperfect_read(rng, mean_code, sd_code, k, int(rng.integers(200, 600)), bool(i % 2), 0.05, 0.03, rna) for i in range(16)]
    four_way(monkeypatch, "rna004 imperfect reads", models["syn9"], "rna004", reads)


def test_polya_reads_take_the_certified_sweeps(models, monkeypatch):
    """every read carries the poly-A tie: the certified prefix of the forward sweep and the certified backward sweep run"""
    reads = SP.reads_for(models, "rna004", 7106, 16, (150, 500), polya=(20, 150))
    _, tms = four_way(monkeypatch, "rna004 poly-A, mode ties", models["syn9"], "rna004", reads)
    assert all(tm["reads_strict"] == len(reads) * 32 for tm in tms.values()), {k: tm["reads_strict"] for k, tm in tms.items()}


def test_in_place_layout_on_a_lowered_budget(models, monkeypatch):
    """the memory budget lowered until the in-place posterior layout is chosen: its record is the same byte record (bit 7 set
    in every lane, not looked at). Status, Z and the integer columns equal the separate layout's bit for bit; the
    probabilities (float LPM stored, not rebuilt) are the oracle's within 1e-6."""
    reads = SP.reads_for(models, "rna004", 7101, 16, (900, 1000))
    want, _ = run(monkeypatch, models["syn9"], "rna004", reads, None, False, 2)
    need = sum(len(r.signal) + 2 for r in reads) * (448 * 12 + 64)
    longest = (max(len(r.signal) for r in reads) + 2 + 32) * (448 * 12 + 64)
    for frac in (0.8, 0.5, 0.3):
        res, tm = run(monkeypatch, models["syn9"], "rna004", reads, None, False, 2, budget=int(max(frac * need, 1.3 * longest)))
        if tm["lp_inplace"] == 1:
            break
    assert tm["lp_inplace"] == 1 and tm["page_rows"] <= 32, tm
    assert np.array_equal(res.status, want.status) and np.array_equal(res.Z.view(np.uint64), want.Z.view(np.uint64))
    m = int(want.seg_offsets[-1])
    assert np.array_equal(res.seg_offsets, want.seg_offsets)
    for col in ("signal_positions", "sequence_positions", "states"):
        assert np.array_equal(getattr(res, col)[:m], getattr(want, col)[:m]), col
    check_oracle(res, oracle_of("rna004 900-1000 bases", models["syn9"], "rna004", reads), "in-place layout")


def test_traceback_block_edge_at_64k_rows(models, monkeypatch):
    """two reads whose T - 1 is 65 536 and 65 537: the traceback's first 64-row block ends on, and one past, a multiple of 64
    rows (pages of 256 rows: the switch is off)"""
    _, mean, sd = synth.read_model_file(model_for(models, "rna004"))
    long = synth.make_reads(7107, 2, "rna004", mean, sd, 6900)
    reads = [fit_length(long[0], 65536), fit_length(long[1], 65537)]
    assert [len(r.signal) for r in reads] == [65536, 65537]
    filler = SP.reads_for(models, "rna004", 7109, 510, (30, 100))   # the ticket opens a session sized for the two long reads
    first, _ = four_way(monkeypatch, "rna004 T-1 = 64k, 64k+1", models["syn9"], "rna004", reads, log_rows=None, filler=filler)
    assert (first.status[:2] == 0).all()


def test_last_five_rows_straddle_a_page(models, monkeypatch):
    """two reads whose rows T - 5 .. T - 1 lie on both sides of a page's first row (T - 1 = 32 k + 1 and 32 k + 2, pages of
    8 .. 32 rows): the fetch cursor reaches its clamp at row T next to its last page crossing"""
    _, mean, sd = synth.read_model_file(model_for(models, "rna004"))
    base = synth.make_reads(7108, 2, "rna004", mean, sd, 330)
    reads = [fit_length(base[0], 32 * 90 + 1), fit_length(base[1], 32 * 90 + 2)]
    first, tms = four_way(monkeypatch, "rna004 last rows across a page", models["syn9"], "rna004", reads)
    assert (first.status == 0).all()
    assert all(tm["page_rows"] <= 32 for tm in tms.values())
