"""The pooled Baum-Welch statistics (csrc/pool_stats.hip: k_pool_fill, k_pool_keys, rocPRIM's radix sort, k_pool_gather,
k_pool_segments) pinned bit for bit.

pool_stats.hip promises "bit for bit the sum dyn_batch_fetch_train forms on the host": columns ascending inside a read, one
partial sum per read, the partial sums in input order. The rest of the suite compares that with rtol 1e-9 (any association
passes) or on five reads. Here tests/device_math/pool_stats.hip, compiled with the product's flags, hands launch_pool_stats
descriptors, codes and column sums built on the host (tests/pool_stats_cases.py), and every bit of pooled[] -- the codes
that occur, the codes that do not (they keep what the array held), the guard behind it -- is compared with the restatement.

Not GPU-marked: that the harness compiles, that the cases have the shape they are named for, and that the inputs can tell a
wrong association, or a launch slice handed the wrong descriptors, from the right one.

No torch in this process (tests/conftest.py, torch_sees_a_gpu: two HIP runtimes)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pool_stats_cases as psc
from conftest import ROOT
from dynamont_amd import _native

gpu = pytest.mark.gpu

SMALL = ["family/%d" % K for K in psc.FAMILY_KMERS] + ["long_run", "runs", "neg_zero"] + ["size/%d" % t for t in psc.SIZES]


@pytest.fixture(scope="module")
def harness_so(tmp_path_factory):
    """tests/device_math/pool_stats.hip -> a shared library, with the flags of every translation unit of the product"""
    so = tmp_path_factory.mktemp("poolstats") / "libpoolstats.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/pool_stats.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd and "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(so)


@pytest.fixture(scope="module")
def cases():
    return psc.small_cases()


@pytest.fixture(scope="module")
def sliced():
    return psc.build_sliced()


@pytest.fixture(scope="module")
def want(cases):
    return {name: psc.reference(c) for name, c in cases.items()}


@pytest.fixture(scope="module")
def sliced_want(sliced):
    return psc.reference(sliced)


@pytest.fixture(scope="module")
def lib(harness_so, native_lib):
    h = C.CDLL(harness_so)
    h.ps_run.restype = C.c_int
    return h


def run_on_device(lib, c):
    """ps_run -> pooled[3 * num_kmers]; every HIP call returned hipSuccess and the three guards still hold the poison"""
    n = 3 * c.num_kmers
    pooled = np.concatenate([c.pooled_init, np.zeros(psc.GUARD)])
    guard = np.zeros(2 * psc.GUARD, dtype=np.uint8)
    err = np.full(64, -1, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    k = lib.ps_run(C.c_int(len(c.read)), p(c.par_off), p(c.N), p(c.read), C.c_int(len(c.status)), p(c.status),
                   C.c_uint64(c.total_cols), p(c.kmers), p(c.col_w), p(c.col_s1), p(c.col_s2), C.c_uint64(c.num_kmers),
                   C.c_int(psc.POISON), p(pooled), p(guard), p(err))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    assert (psc.bits(pooled[n:]) == psc.POISON_U64).all(), "written behind pooled[]"
    assert (guard == psc.POISON).all(), "written behind the work or the temp buffer"
    return pooled[:n]


def mismatch(c, got, want):
    """text for the codes whose bits differ, or None"""
    K = c.num_kmers
    bad = np.flatnonzero(psc.bits(got) != psc.bits(want))
    lines = ["%s[code %d]: device %r (%#x), reference %r (%#x)" % (("w", "s1", "s2")[i // K], i % K, got[i], int(psc.bits(got)[i]),
                                                                    want[i], int(psc.bits(want)[i])) for i in bad[:6]]
    return ("%d of %d differ: " % (len(bad), 3 * K) + "; ".join(lines)) if len(bad) else None


# ---- not GPU-marked ----------------------------------------------------------------------------------------------------------
def test_harness_compiles_with_the_products_flags(harness_so):
    assert os.path.getsize(harness_so) > 0


def test_seq_group_sum_is_a_left_to_right_sum():
    """the vectorised reference against a Python loop, one addition at a time"""
    rng = np.random.default_rng(1)
    keys = rng.integers(0, 7, 200)
    vals = np.ldexp(rng.uniform(1, 2, (3, 200)), rng.integers(-30, 30, 200))
    uniq, sums = psc.seq_group_sum(keys, vals)
    for u, s in zip(uniq, sums.T):
        acc = np.zeros(3)
        for j in np.flatnonzero(keys == u):
            acc = acc + vals[:, j]
        assert np.array_equal(psc.bits(acc), psc.bits(s))


def test_reference_restates_the_host_loop(cases):
    """reference() against finalise_train's loop written out read by read (family/4: failed reads, gaps, a permuted order)"""
    c = cases["family/4"]
    K = c.num_kmers
    pooled = np.zeros(3 * K)
    seen = np.zeros(K, dtype=bool)
    for i in range(len(c.status)):                            # input order
        if not c.has_desc[i] or c.status[i] != 0:
            continue
        a, m = int(c.read_par_off[i]), int(c.read_ncols[i])
        for code in np.unique(c.kmers[a:a + m]):
            w = s1 = s2 = np.float64(0.0)
            for j in range(a, a + m):                         # columns ascending
                if c.kmers[j] == code:
                    w, s1, s2 = w + c.col_w[j], s1 + c.col_s1[j], s2 + c.col_s2[j]
            pooled[code] += w
            pooled[K + code] += s1
            pooled[2 * K + code] += s2
            seen[code] = True
    want = np.where(np.tile(seen, 3), pooled, c.pooled_init)
    assert np.array_equal(psc.bits(psc.reference(c)), psc.bits(want))


def test_cases_hold_what_they_are_named_for(cases, sliced):
    for K in psc.FAMILY_KMERS:
        c = cases["family/%d" % K]
        assert c.num_kmers == K
        ok_cols = c.owned & (c.status[np.repeat(np.arange(len(c.status)), c.read_ncols + np.where(c.has_desc, 0, 3))] == 0)
        used = set(c.kmers[ok_cols].tolist())
        assert 0 in used and K - 1 in used
        assert (len(used) < K) == (K > 128)                                         # codes that never occur keep the initial bits
        assert np.isnan(c.col_w[~c.owned]).all() and (~c.owned).sum() >= 12 and np.isfinite(c.col_w[c.owned]).all()
        assert ((c.kmers[~c.owned] >= 0) & (c.kmers[~c.owned] < K)).all()
        st = c.status[c.read]                                                       # in processing order
        bad = np.flatnonzero(st != 0)
        assert bad[0] == 0 and bad[-1] == len(st) - 1 and ((bad > 0) & (bad < len(st) - 1)).sum() >= 2
        assert c.status[0] != 0 and c.status[-1] != 0                              # and in input order
        assert (np.diff(c.N.astype(np.int64)[st == 0]) <= 0).all()                # by N descending ...
        assert (np.diff(c.par_off.astype(np.int64)) < 0).sum() > len(st) // 4            # ... which is not the input order
        a = int(c.read_par_off[c.repeat_read])
        rc = c.kmers[a:a + 11]
        assert rc[1] == rc[5] == rc[9] and (K == 1 or (np.flatnonzero(rc == rc[1]).tolist() == [1, 5, 9]))
        ok = ok_cols & np.isfinite(c.col_w)
        assert np.log2(c.col_w[ok].max() / c.col_w[ok].min()) > (60 if K > 4 else 0) and c.col_w[ok].min() > 0
        assert (c.col_s1[ok] < 0).any() and (c.col_s1[ok] > 0).any() and (np.signbit(c.col_s1[ok]) & (c.col_s1[ok] == 0)).any()
    w = np.concatenate([cases["family/%d" % K].col_w for K in (1024, 262144)])
    w = w[np.isfinite(w) & (w < 1e299)]
    assert w.min() < 2.0 ** -55 and w.max() > 2.0 ** 19
    assert any(cases["family/%d" % K].total_cols % 2 == 1 for K in psc.FAMILY_KMERS)
    c = cases["long_run"]
    start, n = psc.sorted_runs(c)[c.hot]
    assert n == 298 * 20 and (start + n - 1) // 256 - start // 256 >= 23           # one run over 24 blocks of k_pool_segments
    runs = psc.sorted_runs(cases["runs"])
    assert runs[0][0] == 0 and runs[1] == (255, 1) and runs[2] == (256, 511) and runs[3][0] % 256 == 255 and runs[3][0] > 256
    assert 4 not in runs and 5 in runs
    for t in psc.SIZES:
        assert cases["size/%d" % t].total_cols == t
    assert {1, 255, 256, 257} <= set(psc.SIZES) and any(t % 2 and t > 257 for t in psc.SIZES)
    c = cases["neg_zero"]
    assert np.signbit(c.col_s1[c.kmers == 1]).all() and (c.col_s1[c.kmers == 1] == 0).all()
    assert psc.bits(psc.reference(c))[c.num_kmers + 1] == 0                        # +0.0
    # the 65 541 descriptors
    s = sliced
    assert len(s.read) == psc.SLICE + psc.TAIL and set(np.unique(s.N)) == {2, 3}
    assert np.array_equal(np.sort(s.read[psc.SLICE:]), s.tail_reads) and (s.status[s.tail_reads] == 0).all()
    first = np.zeros(s.total_cols, dtype=bool)
    for k in range(psc.SLICE, len(s.read)):
        a = int(s.par_off[k])
        assert s.kmers[a] < 500 and s.kmers[a + 1] in psc.TAIL_CODES
        first[a:a + 2] = True
    assert not np.isin(s.kmers[~first], psc.TAIL_CODES).any()                      # codes nobody else has
    assert all((s.kmers[~first] == s.kmers[int(s.par_off[k])]).sum() > 20 for k in range(psc.SLICE, len(s.read)))
    assert 1000 < s.tail_reads.min() and s.tail_reads.max() < len(s.read) - 1000   # their partial sums enter in mid-sum
    assert (s.status != 0).sum() == 300


@pytest.mark.parametrize("K", psc.FAMILY_KMERS)
@pytest.mark.parametrize("wrong", psc.WRONG)
def test_inputs_tell_a_wrong_association_apart(cases, want, K, wrong):
    """One flat sum per code, the reads' partial sums in descriptor order, the columns of a read in descending order: each
    differs in bits from the right association in all three statistics, for at least 8 codes (for at least one where the
    table has fewer than 8). A condition on the inputs: a kernel that sums in any of these orders cannot pass."""
    c = cases["family/%d" % K]
    d = psc.differing_codes(c, psc.reference(c, wrong), want[c.name])
    print(c.name, wrong, "codes that differ (w, s1, s2):", d.tolist())
    assert (d >= (8 if K >= 8 else 1)).all(), (wrong, d)


def test_long_run_tells_a_wrong_association_apart(cases, want):
    c = cases["long_run"]
    for wrong in psc.WRONG:
        other = psc.reference(c, wrong)
        assert all(psc.bits(other)[s * c.num_kmers + c.hot] != psc.bits(want[c.name])[s * c.num_kmers + c.hot] for s in range(3)), wrong


def test_inputs_tell_a_wrong_slice_apart(sliced, sliced_want):
    """A second launch of k_pool_keys that is handed the first descriptors again (descs in place of descs + r0) leaves the
    columns of descriptors 65 535 .. 65 540 out: the codes only they have keep the initial bits, the shared ones miss a term."""
    other = psc.reference(sliced, descs=np.concatenate([np.arange(psc.SLICE), np.arange(psc.TAIL)]))
    d = psc.differing_codes(sliced, other, sliced_want)
    assert (d >= 2 * psc.TAIL).all(), d
    K = sliced.num_kmers
    assert (psc.bits(other)[psc.TAIL_CODES] == psc.bits(sliced.pooled_init)[psc.TAIL_CODES]).all()
    assert (psc.bits(sliced_want)[K + psc.TAIL_CODES] != psc.bits(sliced.pooled_init)[K + psc.TAIL_CODES]).all()


# ---- on the device -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", SMALL)
def test_pooled_bit_for_bit(lib, cases, want, name):
    """every bit of pooled[]: the codes that occur, and the initial contents under the codes that do not; a second run of the
    same call leaves the same bits"""
    c = cases[name]
    first = run_on_device(lib, c)
    bad = mismatch(c, first, want[name])
    assert bad is None, (name, bad)
    second = run_on_device(lib, c)
    assert np.array_equal(psc.bits(first), psc.bits(second)), name


@gpu
def test_more_reads_than_one_launch_slice(lib, sliced, sliced_want):
    """65 541 descriptors: k_pool_keys runs a second launch over descriptors 65 535 .. 65 540"""
    got = run_on_device(lib, sliced)
    bad = mismatch(sliced, got, sliced_want)
    assert bad is None, bad
