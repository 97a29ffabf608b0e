"""GPU (-m gpu): which float LPE cells of a lattice row the forward sweep stores (dynamont_amd/csrc/lpe_liveness.hpp).
tests/device_math/lpe_liveness.hip, built with the product's flags, runs lpe_lane_live and lpe_store_mask on rows of the test's
own, one wave per row; both masks of every row must equal a three-line NumPy restatement of the definition:
  a lane is live when any of its seven cells has not (f < floor); all sixteen lanes of a group with a live lane store."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from dynamont_amd import _native

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("native_lib")]

FLOOR = np.float32(-750.0)
DEAD = np.float32(-800.0)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("lpelive") / "liblpelive.so"
    cmd = [_native.hipcc_path()] + _native.hipcc_flags() + ["-I", _native.CSRC, "-shared", "-x", "hip",
                                                            str(ROOT) + "/tests/device_math/lpe_liveness.hip", "-o", str(so)]
    assert "--offload-arch=gfx950" in cmd
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    lib = C.CDLL(str(so))
    lib.lv_run.restype = C.c_int
    return lib


def restate(rows, floor):
    """(live lanes, store-live lanes) of every row as 64-bit masks: the definition, in float32 like the kernel"""
    with np.errstate(invalid="ignore"):
        lanes = (~(rows.reshape(-1, 64, 7) < np.float32(floor))).any(axis=2)                  # NaN: not (NaN < floor)
    groups = np.repeat(lanes.reshape(-1, 4, 16).any(axis=2), 16, axis=1)
    pack = lambda m: (m.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)  # noqa: E731
    return pack(lanes), pack(groups)


def run(lib, rows, floor):
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    out = np.zeros(2 * len(rows), dtype=np.uint64)
    err = np.full(16, -1, dtype=np.int32)
    k = lib.lv_run(C.c_int(len(rows)), rows.ctypes.data_as(C.c_void_p), C.c_float(float(floor)), out.ctypes.data_as(C.c_void_p),
                   err.ctypes.data_as(C.c_void_p))
    assert k > 0 and not err[:k].any(), ("hipError_t of every step", k, err[:max(k, 0)].tolist())
    return out[0::2], out[1::2]


def crafted_rows():
    rows, what = [], []

    def add(row, label):
        rows.append(row)
        what.append(label)

    dead = np.full(448, DEAD, dtype=np.float32)
    add(dead.copy(), "all cells dead")
    add(np.full(448, -np.inf, dtype=np.float32), "all cells -inf")
    below, above = np.nextafter(FLOOR, np.float32(-np.inf)), np.nextafter(FLOOR, np.float32(0))
    # one special cell in the first and the last lane of every group, in the first, a middle and the last cell of the lane
    for lane in (0, 15, 16, 31, 32, 47, 48, 63):
        for cell in (0, 3, 6):
            for v, label in ((np.float32(-1.0), "live"), (FLOOR, "at the floor"), (below, "just below the floor"),
                             (above, "just above the floor"), (np.float32(np.nan), "NaN"), (np.float32(-np.inf), "-inf"),
                             (np.float32(0.0), "zero"), (np.float32(3.0e-7), "rounded above 0")):
                r = dead.copy()
                r[lane * 7 + cell] = v
                add(r, f"{label} in lane {lane} cell {cell}")
    nan_neg = np.array([0xffc00001], dtype=np.uint32).view(np.float32)[0]           # a NaN with the sign bit set
    r = dead.copy()
    r[20 * 7 + 2] = nan_neg
    add(r, "negative NaN")
    r = dead.copy()
    r[5 * 7:6 * 7] = [np.nan, DEAD, -np.inf, DEAD, np.nan, DEAD, DEAD]              # NaN beside dead cells in all three maxima
    add(r, "NaN among dead cells")
    r = dead.copy()
    r[15 * 7 + 6] = -1.0
    r[16 * 7] = -2.0
    add(r, "two groups, neighbours across the group border")
    r = dead.copy()
    r[[0, 447]] = -1.0
    add(r, "first and last slot of the row")
    add(np.full(448, -1.0, dtype=np.float32), "every cell live")
    rng = np.random.default_rng(77)
    for k in range(40):                                                               # a few live cells anywhere
        r = dead.copy()
        r[rng.integers(0, 448, size=int(rng.integers(1, 5)))] = rng.uniform(-760.0, -740.0, size=1).astype(np.float32)
        add(r, f"random {k}")
    return np.stack(rows), what


def test_masks_equal_the_restatement(harness):
    rows, what = crafted_rows()
    for floor in (FLOOR, np.float32(-5.0), np.float32(-np.inf)):
        want_lanes, want_groups = restate(rows, floor)
        got_lanes, got_groups = run(harness, rows, floor)
        bad = np.flatnonzero((got_lanes != want_lanes) | (got_groups != want_groups))
        assert bad.size == 0, [(float(floor), what[i], hex(int(got_lanes[i])), hex(int(want_lanes[i])), hex(int(got_groups[i])),
                                hex(int(want_groups[i]))) for i in bad[:6]]
    # what the restatement itself says about the corner cases (so that a wrong restatement cannot hide a wrong kernel)
    lanes, groups = restate(rows, FLOOR)
    at = {w: i for i, w in enumerate(what)}
    assert lanes[at["all cells dead"]] == 0 and groups[at["all cells -inf"]] == 0
    assert groups[at["at the floor in lane 15 cell 6"]] == 0xffff and groups[at["just above the floor in lane 16 cell 0"]] == 0xffff0000
    assert groups[at["just below the floor in lane 0 cell 0"]] == 0 and groups[at["-inf in lane 63 cell 6"]] == 0
    assert lanes[at["NaN in lane 63 cell 3"]] == 1 << 63 and groups[at["NaN in lane 63 cell 3"]] == 0xffff << 48
    assert groups[at["negative NaN"]] == 0xffff0000 and groups[at["NaN among dead cells"]] == 0xffff
    assert groups[at["two groups, neighbours across the group border"]] == 0xffffffff
    assert groups[at["first and last slot of the row"]] == 0xffff00000000ffff
    # the dense switch: floor = -inf stores every lane of every row, the all -inf row included
    _, dense = run(harness, rows, np.float32(-np.inf))
    assert (dense == np.uint64(0xffffffffffffffff)).all()
