"""GPU (-m gpu): per-border credible intervals (Aligner.set_border_interval, interval_kernels.hpp). Whole reads through every
place a lattice lives -- the separate layout (plain and certified reads), the in-place layout, a page-starved pool, the
banded-lattice kernel -- against the NumPy restatement over the CPU oracle's lattices (tests/border_interval_cases.py): border_lo
and border_hi by its acceptance rule, border_mean and the variance within the bounds it derives, no border left out. The two
sweeps also run, compiled into a test unit with the product's flags, on a lattice the test writes itself (610 columns,
out-of-band slots poisoned with probability 1, a column whose mass never reaches a threshold): bit for bit the host's sums of the
device's own terms. Switching the intervals on moves nothing else, and off is the launch it has always been."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import border_confidence_cases as bcc
import border_interval_cases as bic
from conftest import ROOT, model_for
from dynamont_amd import Aligner, _native, synth, zstd_io
from dynamont_amd.segmentation import segment as seg

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

COLS = ("border_lo", "border_hi", "border_mean", "border_sd")


@pytest.fixture(scope="module")
def sets(models):
    return bic.read_sets(models)


@pytest.fixture(scope="module")
def yards(models, sets, oracle_built):
    cache = {}
    return lambda name: bic.make_yards(models, sets, name, cache)


def run(model, pore, band, reads, mass, budget=None, rescale=0):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    if rescale:
        al.set_rescale(rescale)
    al.set_border_interval(mass)
    with al.batch([r.signal for r in reads], [r.sequence for r in reads]) as b:
        b.align(True)
        res = b.fetch()
        tm = b.timing()
    al.close()
    return res, tm


def run_off(model, pore, band, reads, budget=None):
    al = Aligner(model, pore, band=band, device=0)
    if budget:
        al.set_mem_budget(budget)
    res = al.align_batch([r.signal for r in reads], [r.sequence for r in reads], True)
    assert all(getattr(res, c) is None for c in COLS) and "border_lo" not in res.read(0)
    al.close()
    return res


def check(res, ys, mass, what):
    assert (res.status[:len(ys)] == 0).all(), (what, res.status)
    assert res.border_lo.dtype == res.border_hi.dtype == np.uint32 and res.border_mean.dtype == res.border_sd.dtype == np.float64
    for i, y in enumerate(ys):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        assert m == y.N - 1 and np.array_equal(res.signal_positions[a:a + m], y.res["signal_positions"]), (what, i)
        bic.check_device(y, mass, *(getattr(res, c)[a:a + m] for c in COLS), f"{what} read {i}")


def same_segments(a, b):
    """no segment, Z or probability moved"""
    assert np.array_equal(a.status, b.status)
    assert np.array_equal(a.Z.view(np.uint64), b.Z.view(np.uint64))
    assert np.array_equal(a.n_segments, b.n_segments) and np.array_equal(a.seg_offsets, b.seg_offsets)
    m = int(a.seg_offsets[-1])
    for col in ("signal_positions", "sequence_positions", "probabilities"):
        assert np.array_equal(getattr(a, col)[:m].view(np.uint64), getattr(b, col)[:m].view(np.uint64)), col


def same_intervals(a, b):
    m = int(a.seg_offsets[-1])
    for c in COLS:
        x, y = getattr(a, c)[:m], getattr(b, c)[:m]
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), c


# ---- 1. separate layout, plain and certified reads --------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", bic.MASSES)
@pytest.mark.parametrize("name", ["plain", "imperfect"])
def test_separate_layout(models, sets, yards, name, mass):
    """plain: rna004 reads, the plain launch; imperfect: rna002 reads (pad + A, a structural tie at the read's start) -- the
    launch that carries both arithmetic flavours."""
    key, pore, band, reads = sets[name]
    ys = yards(name)
    if mass == 0.9:
        bic.assert_conditions(ys, name)
    res, tm = run(models[key], pore, band, reads, mass)
    assert tm["lp_inplace"] == 0 and tm["launches"] == 1
    if name == "imperfect":
        assert tm["reads_strict"] == len(reads)
    check(res, ys, mass, f"{name} separate")
    d = res.read(1)
    a, m = int(res.seg_offsets[1]), int(res.n_segments[1])
    for c in COLS:
        assert np.array_equal(d[c], getattr(res, c)[a:a + m])
    if mass == 0.9:
        same_segments(res, run_off(models[key], pore, band, reads))


# ---- 2. band 50; 3. slot wrapping and page crossings ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["plain_band50", "imperfect_band50", "long", "long_band50"])
def test_narrow_band_and_wrapping_slots(models, sets, yards, name):
    """band 50: most of a lane's slots hold no column, and on the imperfect reads the path runs along the band's edge, where an
    unmasked read of a slot would gain mass. The 700-base reads have 693 lattice columns: a band slot is n mod 448, so slots wrap
    and a lane hands a finished column over for the next one; their ~6 900 rows span several pages. At band 400 and at band 50."""
    key, pore, band, reads = sets[name]
    ys = yards(name)
    if name.startswith("long"):
        assert all(y.N > 448 for y in ys)
    bic.assert_conditions(ys if not name.startswith("long") else yards("long") + yards("long_band50"), name)
    res, _ = run(models[key], pore, band, reads, 0.9)
    check(res, ys, 0.9, name)


# ---- 4. in-place layout and a page-starved pool --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["inplace", "page_starved"])
@pytest.mark.parametrize("name", ["plain", "imperfect_band50", "long_band50"])
def test_inplace_layout_and_page_starved_pool(models, sets, yards, monkeypatch, name, path):
    key, pore, band, reads = sets[name]
    ys = yards(name)
    budget = None
    if path == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    else:
        # a read's lattice takes ~(448 * 8 + 56) bytes per row: room for a fifth of the batch, and for the longest read one and a
        # half times over
        lens = sorted((len(r.signal) for r in reads), reverse=True)
        budget = int(max(0.2 * sum(lens), 1.5 * lens[0]) * (448 * 8 + 56))
    res, tm = run(models[key], pore, band, reads, 0.9, budget=budget)
    off = run_off(models[key], pore, band, reads, budget)
    if path == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
        assert tm["lp_inplace"] == 1
        if name.startswith("imperfect"):
            assert tm["reads_strict"] == len(reads)                 # in place AND both flavours: k_read_queue<JOB_ALIGN_INPLACE | JOB_INTERVAL, true>
    else:
        print(f"{name} page-starved: pool_pages {tm['pool_pages']}, page_rows {tm['page_rows']}, n_static {tm['n_static']} of {len(reads)}")
    check(res, ys, 0.9, f"{name} {path}")
    same_segments(res, off)


# two of the six "plain" reads carry a tie by chance (dyn_tie_rows), so every batch above takes the launch with both arithmetic
# flavours; these four carry none
PLAIN_WITHOUT_A_TIE = (1, 2, 4, 5)


@pytest.mark.parametrize("layout", ["separate", "inplace"])
def test_launch_without_a_certified_read(models, sets, yards, monkeypatch, layout):
    """k_read_queue<JOB_ALIGN | JOB_INTERVAL, false> and <JOB_ALIGN_INPLACE | JOB_INTERVAL, false>: a batch the tie rule flags no
    read of, held as the batches above are"""
    key, pore, band, reads = sets["plain"]
    reads, ys = [reads[i] for i in PLAIN_WITHOUT_A_TIE], [yards("plain")[i] for i in PLAIN_WITHOUT_A_TIE]
    if layout == "inplace":
        monkeypatch.setenv("DYN_FORCE_LAYOUT", "inplace")
    res, tm = run(models[key], pore, band, reads, 0.9)
    off = run_off(models[key], pore, band, reads)
    if layout == "inplace":
        monkeypatch.delenv("DYN_FORCE_LAYOUT")
    assert tm["lp_inplace"] == (1 if layout == "inplace" else 0) and tm["launches"] == 1 and tm["reads_strict"] == 0
    check(res, ys, 0.9, f"plain without a tie, {layout}")
    same_segments(res, off)


# ---- 5. the banded-lattice kernel ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def wide(models, oracle_built):
    from oracle.pyoracle import Oracle
    reads = bcc.plain_reads(models["syn5"], "rna002", bcc.WIDE_SEED, 1, 600)
    orc = Oracle(models["syn5"], synth.PORES["rna002"][0], 600)
    return reads, [bic.Yard(orc, reads[0].signal, reads[0].sequence, 600)]


@pytest.mark.parametrize("mass", [0.5, 0.999])
def test_banded_lattice_kernel(models, wide, mass):
    """one rna002 read of 600 bases at band = 600: half band 298, above the register sweeps' 223 (band_reads.hip)"""
    reads, ys = wide
    assert min(600 // 2, (len(reads[0].sequence) - 5 + 2) // 2) == 298
    res, _ = run(models["syn5"], "rna002", 600, reads, mass)
    check(res, ys, mass, "wide")
    if mass == 0.5:
        same_segments(res, run_off(models["syn5"], "rna002", 600, reads))


# ---- 6. reproducible, the same through a ticket, the last pass's with rescaling ------------------------------------------------
def test_runs_and_tickets(models, sets, yards):
    key, pore, band, reads = sets["plain"]
    first, _ = run(models[key], pore, band, reads, 0.9)
    again, _ = run(models[key], pore, band, reads, 0.9)
    same_intervals(first, again)                                            # two runs: identical bits
    al = Aligner(models[key], pore, band=band, device=0)
    al.set_border_interval(0.9)
    t = al.align_async(*synth.pack_reads(reads), True)
    res = t.wait()
    same_segments(res, first)
    same_intervals(res, first)                                              # an asynchronous ticket: the same bits as align_batch
    assert t.timing()["launches"] >= 1
    m = int(res.seg_offsets[-1])
    lo, hi = np.zeros(m + 5, dtype=np.uint32), np.zeros(m + 5, dtype=np.uint32)
    mean, sd = np.zeros(m + 5), np.zeros(m + 5)
    p32, p64 = (lambda x: x.ctypes.data_as(_native.c_u32_p)), (lambda x: x.ctypes.data_as(_native.c_double_p))
    t.fetch_intervals(_native.DynBorderIntervalOut(p32(lo), p32(hi), p64(mean), p64(sd), m + 5))
    assert np.array_equal(lo[:m], res.border_lo[:m]) and np.array_equal(sd[:m], res.border_sd[:m]) and not lo[m:].any()
    with pytest.raises(ValueError, match="capacity"):
        t.fetch_intervals(_native.DynBorderIntervalOut(p32(lo), p32(hi), p64(mean), p64(sd), m - 1))
    t.close()
    al.close()
    # with rescaling the values are the last pass's: the intervals lie about the borders that pass called
    resc, tm = run(models[key], pore, band, reads, 0.9, rescale=1)
    m = int(resc.seg_offsets[-1])
    assert (resc.border_lo[:m] <= resc.signal_positions[:m] + 64).all() and (resc.border_lo[:m] <= resc.border_hi[:m]).all()
    assert np.abs(resc.border_mean[:m] - resc.signal_positions[:m]).max() < 64


# ---- 7. a failed read and a read of N = 2 --------------------------------------------------------------------------------------
def test_failed_read_and_two_column_read(models, sets, yards):
    key, pore, band, reads = sets["plain"]
    tiny = bcc.plain_reads(models[key], pore, 31, 1, 9)[0]                  # 9 bases at k = 9: N = 2, one output row
    failed = synth.SynthRead(reads[1].signal, reads[1].sequence[:40] + "N" + reads[1].sequence[41:])   # fails validation
    batch = [reads[0], failed, tiny, reads[2]]
    res, _ = run(models[key], pore, band, batch, 0.9)
    assert res.status[1] != 0 and (res.status[[0, 2, 3]] == 0).all() and res.n_segments[2] == 1
    a = int(res.seg_offsets[2])
    # the one border there is: forced, row 1 holds the whole mass
    assert res.border_lo[a] == 0 and res.border_hi[a] == 0 and abs(res.border_mean[a]) <= 1e-6 and res.border_sd[a] <= 1e-3
    lo, hi = int(res.seg_offsets[1]), int(res.seg_offsets[2])
    for c in COLS:
        assert not getattr(res, c)[lo:hi].any()                             # rows of the failed read stay 0
    ys = yards("plain")
    for i, j in ((0, 0), (3, 2)):
        a, m = int(res.seg_offsets[i]), int(res.n_segments[i])
        bic.check_device(ys[j], 0.9, *(getattr(res, c)[a:a + m] for c in COLS), f"mixed batch read {i}")


# ---- 8. the switch is per ticket, merges with its like, and changes nothing else ------------------------------------------------
def test_switch_is_per_ticket_and_changes_nothing_else(models):
    _, mean, sd = synth.read_model_file(models["syn9"])
    data = [synth.make_reads(7600 + j, 600, "rna004", mean, sd, (60, 120)) for j in range(2)]
    never = Aligner(models["syn9"], "rna004", device=0)                     # a handle that never switched it on
    base = [never.align_batch([r.signal for r in reads], [r.sequence for r in reads], True) for reads in data]
    never.close()
    al = Aligner(models["syn9"], "rna004", device=0)
    plan = [(0, 0), (0.9, 1), (0.5, 0), (0, 1), (0.9, 1)]                   # (mass, data set), in submission order
    tickets = []
    for mass, k in plan:
        al.set_border_interval(mass)
        tickets.append(al.align_async(*synth.pack_reads(data[k]), True))
    al.set_border_interval(0)
    results = []
    for (mass, k), t in zip(plan, tickets):
        res = t.wait()
        results.append(res)
        same_segments(res, base[k])                                         # start, Z and probabilities: bit-equal to a plain run
        launches = t.timing()["launches"]
        if mass == 0:
            assert res.border_lo is None
            assert launches == 0                                            # published into the resident session (600 reads)
            u, d = np.zeros(int(res.cap), dtype=np.uint32), np.zeros(int(res.cap))
            with pytest.raises(ValueError, match="without dyn_aligner_set_border_interval"):
                t.fetch_intervals(_native.DynBorderIntervalOut(u.ctypes.data_as(_native.c_u32_p), u.ctypes.data_as(_native.c_u32_p),
                                                               d.ctypes.data_as(_native.c_double_p), d.ctypes.data_as(_native.c_double_p), int(res.cap)))
        else:
            assert launches >= 1                                            # a launch of its own: no session
            m = int(res.seg_offsets[-1])
            assert (res.border_lo[:m] <= res.border_hi[:m]).all() and (res.border_sd[:m] >= 0).all()
            inside = (res.border_lo[:m] <= res.signal_positions[:m]) & (res.signal_positions[:m] <= res.border_hi[:m])
            print(f"mass {mass}: the called border lies inside its interval on {100 * inside.mean():.1f} % of {m} borders")
            assert inside.mean() >= mass / 2                                # (a plausibility check: the called border is where the mass is)
    same_intervals(results[1], results[4])                                  # two tickets of the same reads and mass: the same bits
    for t in tickets:
        t.close()
    st = al.session_stats()
    assert st["sessions"] >= 1 and st["aborted"] == 0
    al.close()


def test_refusals(models, sets):
    key, pore, band, reads = sets["plain"]
    sig, seq = [r.signal for r in reads[:3]], [r.sequence for r in reads[:3]]
    al = Aligner(models[key], pore, device=0)
    u, d = np.zeros(4096, dtype=np.uint32), np.zeros(4096)
    mk = lambda cap: _native.DynBorderIntervalOut(u.ctypes.data_as(_native.c_u32_p), u.ctypes.data_as(_native.c_u32_p),  # noqa: E731
                                                  d.ctypes.data_as(_native.c_double_p), d.ctypes.data_as(_native.c_double_p), cap)
    with al.batch(sig, seq) as b:
        b.align(True)                          # switch off at submission
        al.set_border_interval(0.9)
        with pytest.raises(ValueError, match="without dyn_aligner_set_border_interval"):
            b.fetch_intervals(mk(4096))
        b.align(False)                         # Z only, switch on
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_intervals(mk(4096))
        b.train()
        with pytest.raises(ValueError, match="calc_probabilities"):
            b.fetch_intervals(mk(4096))
        b.align(True)
        b.fetch_intervals(mk(4096))
        with pytest.raises(ValueError, match="capacity"):
            b.fetch_intervals(mk(3))
        for on, off, word in ((lambda: al.set_border_confidence(8), lambda: al.set_border_confidence(0), "dyn_aligner_set_border_confidence"),
                              (lambda: al.set_posterior_samples(4, 1), lambda: al.set_posterior_samples(0), "dyn_aligner_set_posterior_samples"),
                              (lambda: al.set_guide_rescue(4, 16), lambda: al.set_guide_rescue(0, 0), "dyn_aligner_set_guide_rescue")):
            on()
            with pytest.raises(ValueError, match="dyn_batch_align: dyn_aligner_set_border_interval is on, which does not combine with " + word):
                b.align(True)
            with pytest.raises(ValueError, match="dyn_batch_align_async: dyn_aligner_set_border_interval is on, which does not combine with " + word):
                al.align_async(*synth.pack_reads(reads[:3]), True)
            off()
        al.set_auto_guide(16)
        with pytest.raises(ValueError, match="dyn_aligner_set_border_interval is on, which does not combine with dyn_aligner_set_auto_guide"):
            al.align_async(*synth.pack_reads(reads[:3]), True)
        al.set_auto_guide(0)
        b.align(True)                          # every other switch off again: accepted
    with pytest.raises(ValueError, match="carries a guide"):
        al.align_batch_auto(sig, seq, 16, 1)
    with pytest.raises(ValueError, match="mass must be 0 or"):
        al.set_border_interval(1.5)
    assert al._border_interval == 0.9
    al.close()


# ---- 9. through the sink and the command line ------------------------------------------------------------------------------------
def test_through_the_sink(models, sets, tmp_path):
    key, pore, band, reads = sets["plain"]
    reads = reads[:3]
    al = Aligner(models[key], pore, device=0)
    L = _native.lib()
    h = C.c_void_p()
    err = C.create_string_buffer(1024)
    assert L.dyn_csv_sink_open_ex(str(tmp_path / "o.csv.zst").encode(), str(tmp_path / "o.errors").encode(), 3, 1, 1, 1,
                                  _native.DYN_CSV_BORDER_INTERVAL, C.byref(h), err, 1024) == 0, err.value
    sig, sig_off, seqs, seq_off = synth.pack_reads(reads)
    n = len(reads)
    rid = (C.c_char_p * n)(*[f"r{i}".encode() for i in range(n)])
    sid = (C.c_char_p * n)(*[f"s{i}".encode() for i in range(n)])
    starts = np.full(n, 100, dtype=np.int64)                                # the reads' aligned slices start at sample 100
    lengths = np.diff(np.asarray(sig_off).astype(np.int64)).astype(np.uint64)
    so = np.ascontiguousarray(seq_off, dtype=np.uint64)

    def submit(t):
        return L.dyn_csv_sink_submit(h, al._h, t._h, C.byref(t.result._c), n, seqs, so.ctypes.data_as(_native.c_u64_p), rid, sid,
                                     starts.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(_native.c_u64_p))

    lacking = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(lacking) == _native.DYN_ERR_INVALID_ARGUMENT and "DYN_CSV_BORDER_INTERVAL" in al.last_error()
    al.set_border_interval(0.9)
    on = al.align_async(sig, sig_off, seqs, seq_off, True)
    assert submit(on) == 0
    assert L.dyn_csv_sink_wait(h, 1, -1) == 1
    csv, zst, nerr = C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert L.dyn_csv_sink_close(h, C.byref(csv), C.byref(zst), C.byref(nerr), err, 1024) == 0, err.value
    lines = zstd_io.decompress(open(tmp_path / "o.csv.zst", "rb").read()).split(b"\n")
    assert lines[0].endswith(b",polish,border_lo,border_hi,border_mean,border_sd")
    res = on.wait()
    assert len(lines) - 2 == int(res.n_segments.sum())
    for j in (0, 1, int(res.n_segments[0]) - 1, int(res.n_segments[0])):
        fields = lines[1 + j].split(b",")
        want = f"{int(res.border_lo[j]) + 100},{int(res.border_hi[j]) + 100},{res.border_mean[j] + 100.0:.6f},{res.border_sd[j]:.6f}"
        assert b",".join(fields[-4:]) == want.encode(), (j, lines[1 + j])
        assert int(fields[2]) == int(res.signal_positions[j]) + 100        # the `start` column: the same unit
    lacking.close()
    on.close()
    al.close()


def _cli(model, pore, raw, bam, out, *extra):
    seg.main(["-r", os.path.dirname(raw), "-b", bam, "--mode", "basic", "-p", pore, "--model_path", model,
              "--batch-reads", "4", "-o", str(out)] + list(extra))
    data = open(str(out) + ".zst", "rb").read()
    errors = os.path.splitext(str(out))[0] + ".errors"
    return zstd_io.decompress(data).decode(), open(errors).read() if os.path.exists(errors) else ""


def test_command_line(models, tmp_path):
    """dynamont-resquiggle --border-interval 0.9 on a small file: four more fields per row, everything before them the run
    without the flag; the Python formatting path writes the same bytes; 0 is off"""
    pore = "rna004"
    model = model_for(models, pore)
    _, mean, sd = synth.read_model_file(model)
    reads = synth.make_reads(7511, 6, pore, mean, sd, (60, 160))
    raw, bam, _ = synth.write_dataset(str(tmp_path / "in"), "bi", reads, pore, seed=3, basecalls="tsv")
    plain, plain_err = _cli(model, pore, raw, bam, tmp_path / "plain.csv")
    text, err = _cli(model, pore, raw, bam, tmp_path / "bi.csv", "--border-interval", "0.9")
    assert err == plain_err
    b_lines, s_lines = plain.splitlines(), text.splitlines()
    assert s_lines[0] == b_lines[0] + ",border_lo,border_hi,border_mean,border_sd" and len(b_lines) == len(s_lines) > 100
    inside = 0
    for b, s in zip(b_lines[1:], s_lines[1:]):
        f = s.split(",")
        assert ",".join(f[:-4]) == b                    # everything before the new fields: the run without the flag
        lo, hi, mean_, sd_ = int(f[-4]), int(f[-3]), float(f[-2]), float(f[-1])
        assert lo <= hi and sd_ >= 0 and mean_ >= 0 and re_fixed6(f[-2]) and re_fixed6(f[-1])
        inside += lo <= int(f[2]) <= hi                  # the `start` column's unit
    assert inside >= 0.45 * (len(s_lines) - 1)           # (a plausibility check: the called border is where the mass is)
    frames, frames_err = _cli(model, pore, raw, bam, tmp_path / "frames.csv", "--border-interval", "0.9", "--parallel-zstd-frames")
    assert frames == text and frames_err == err          # the Python formatting path writes the same bytes
    off, off_err = _cli(model, pore, raw, bam, tmp_path / "off.csv", "--border-interval", "0")
    assert off == plain and off_err == plain_err
    assert open(tmp_path / "off.csv.zst", "rb").read() == open(tmp_path / "plain.csv.zst", "rb").read()


def re_fixed6(text):
    whole, _, frac = text.partition(".")
    return whole.lstrip("-").isdigit() and len(frac) == 6 and frac.isdigit()


# ---- 10. the device harness -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("bint") / "libbint.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/border_interval.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.bi_run.restype = C.c_int
    return lib


P_SLOTS, CPL = 448, 7
POISON = 0.0       # log-posterior 0: probability 1 -- a sweep that read an out-of-band slot would gain a whole unit of mass


def row_pos(s):
    lane, j = s // CPL, s % CPL
    return (j >> 1) * 128 + lane * 2 + (j & 1) if j < 6 else 384 + lane


class Lattice:
    """a read of T rows and N = 610 columns (slots wrap) with a narrow band, in all three layouts: random float log-posteriors of
    a size at which a column's mass passes the thresholds somewhere inside its band interval, -inf cells among them, every slot
    outside the band poisoned. Column `faint` holds so little mass that no threshold is ever reached (in the layouts that store
    LPM; the separate layout rebuilds LPM from its neighbours' LPE, so there the column before it is dead instead)."""

    def __init__(self, seed=17, T=1500, N=610, bw=12, faint=301):
        rng = np.random.default_rng(seed)
        self.T, self.N, self.bw, self.faint = T, N, bw, faint
        self.ratio = N / T
        self.Zb, self.m1 = -1234.5678, 0.0
        self.rowmap = rng.permutation(T + 1).astype(np.uint32)
        B = 2 * bw + 3
        self.lp_in = np.full((T + 1, P_SLOTS, 2), POISON, dtype=np.float32)
        self.lp_wide = np.full((T, B, 2), POISON, dtype=np.float32)
        self.lpe_sep = np.full((T + 1, P_SLOTS), POISON, dtype=np.float32)
        self.bE = np.full((T + 1, P_SLOTS), -1000.0)
        mean, sd = rng.normal(0.0, 0.05, N - 1), rng.uniform(0.3, 0.6, N - 1)
        self.sig = rng.normal(0.0, 0.2, T - 1)
        self.par = np.stack([mean, 1.0 / sd, -np.log(sd), sd], axis=1).copy()
        self.start = np.array([int(t * self.ratio) - bw for t in range(T)], dtype=np.int64)
        self.inband = np.zeros((T + 2, N + 1), dtype=bool)
        for t in range(1, T):
            self.inband[t, max(self.start[t], 1):min(self.start[t] + 2 * bw + 1, N)] = True
        self.rows = np.zeros(N - 1, dtype=np.uint32)
        for n in range(1, N):
            ts = np.nonzero(self.inband[:, n])[0]
            self.rows[n - 1] = ts[len(ts) // 2]                              # r: somewhere inside the column's interval
        for t in range(1, T):
            s = int(self.start[t])
            for n in range(max(s, 1), min(s + 2 * bw + 1, N)):
                # a column is in band for ~60 rows: masses of about 1/30 each pass 0.05 and 0.95 inside the interval
                vm = np.float32(-np.inf) if rng.random() < 0.02 else np.float32(-3.4 - rng.exponential(0.7))
                ve = np.float32(-np.inf) if rng.random() < 0.003 else np.float32(-rng.exponential(0.5))
                if n == faint:
                    vm = np.float32(-12.0 - rng.exponential(1.0))
                if n == faint - 1:
                    ve = np.float32(-np.inf)
                pos = row_pos(n % P_SLOTS)
                self.lp_in[self.rowmap[t], pos] = (vm, ve)
                self.lp_wide[t, n - s + 1] = (vm, ve)
                self.lpe_sep[self.rowmap[t], pos] = ve
                self.bE[self.rowmap[t], pos] = -np.inf if ve == -np.inf else -1000.0 - 0.01 * t + rng.uniform(-0.3, 0.3)


@pytest.fixture(scope="module")
def lattice():
    return Lattice()


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_device_harness_sweeps(harness, lattice, mode):
    """interval_kernels.hpp's wave sweep over the three accessors (modes 0 - 2: separate, in place, wide) and its column walk
    (mode 3, wide) on a lattice of the test's own: 610 columns, a band of 25, every out-of-band slot poisoned with probability 1,
    -inf cells inside the band, one column whose mass never reaches a threshold. lo, hi, S, A and B equal, bit for bit, the host's
    sums of the device's own terms in ascending row order; the terms of the layouts that store a float LPM are exp of exactly that
    float, within 4 ulps."""
    la = lattice
    mass = 0.9
    tail = (1.0 - mass) / 2
    cols, W = la.N - 1, 2 * la.bw + 1
    FILL = 0xABCD1234
    lo, hi = np.full(cols, FILL, dtype=np.uint32), np.full(cols, FILL, dtype=np.uint32)
    sab = np.full((3, cols), -7.0)
    terms = np.full((la.T, W), -7.0)
    err = np.full(64, -1, dtype=np.int32)
    lp = (la.lpe_sep, la.lp_in, la.lp_wide, la.lp_wide)[mode]
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = harness.bi_run(C.c_int(mode), C.c_int(la.T), C.c_int(la.N), C.c_int(la.bw), C.c_double(la.ratio), C.c_double(la.Zb),
                       C.c_double(la.m1), C.c_double(tail), C.c_uint64(la.rowmap.size), p(la.rowmap), C.c_uint64(lp.size), p(lp),
                       C.c_uint64(la.bE.size), p(la.bE), C.c_uint64(la.sig.size), p(la.sig), C.c_uint64(la.par.shape[0]), p(la.par),
                       p(la.rows), p(lo), p(hi), p(sab), p(terms), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    # the terms: written for exactly the in-band cells, and for a stored float LPM exp of that float
    for t in range(1, la.T):
        s = int(la.start[t])
        n = s + np.arange(W)
        ib = (n >= 1) & (n < la.N)
        assert (terms[t, ib] != -7.0).all() and (terms[t, ~ib] == -7.0).all(), t
        assert (terms[t, ib] >= 0.0).all() and np.isfinite(terms[t, ib]).all(), t
        if mode != 0:
            assert (terms[t, ib] < 0.05).all(), t                                   # nothing poisoned: every mass stays small
            want = np.exp(la.lp_wide[t, 1:W + 1, 0].astype(np.float64))[ib]
            assert np.allclose(terms[t, ib], want, rtol=1e-15, atol=0.0), t
    assert (terms[0] == -7.0).all()
    q_lo, q_hi = tail, 1.0 - tail
    never = 0
    for n in range(1, la.N):
        ts = np.nonzero(la.inband[:la.T, n])[0]
        r = int(la.rows[n - 1])
        C_ = A_ = B_ = 0.0
        t_lo = t_hi = 0
        for t in ts.tolist():
            pm = float(terms[t, n - int(la.start[t])])
            d = float(t - r)
            C_ = C_ + pm
            A_ = A_ + d * pm
            B_ = B_ + (d * d) * pm
            t_lo = t if (not t_lo and C_ >= q_lo) else t_lo
            t_hi = t if (not t_hi and C_ >= q_hi) else t_hi
        never += not t_hi
        want_lo, want_hi = (t_lo or int(ts[-1])) - 1, (t_hi or int(ts[-1])) - 1
        assert (int(lo[n - 1]), int(hi[n - 1])) == (want_lo, want_hi), (mode, n, int(lo[n - 1]), int(hi[n - 1]), want_lo, want_hi)
        got = sab[:, n - 1]
        assert np.array_equal(got.view(np.uint64), np.array([C_, A_, B_]).view(np.uint64)), (mode, n, got.tolist(), (C_, A_, B_))
    assert never >= 1                                                         # the column whose mass never reaches 1 - a
    if mode != 0:
        assert sab[0, la.faint - 1] < tail and lo[la.faint - 1] == hi[la.faint - 1]   # ... nor a: both fall back to the last row
    else:
        assert sab[0, la.faint - 1] == 0.0                                    # the separate layout: its predecessors are dead
    print(f"mode {mode}: {cols} columns bit for bit, {never} whose mass never reaches 1 - a")
