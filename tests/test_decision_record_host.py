"""CPU: the per-row record of the forward sweep (dynamont_amd/csrc/decision_record.hpp) compiled for the host with g++.

A row's record is 64 bytes, one per lane of the sweep: bit j (j < 7) of byte l is the traceback decision of band slot
7 l + j, bit 7 says that the lane's float LPE cells of the row were stored. The sweep packs the byte, the traceback and the
segment-start posteriors unpack it: both directions against a Python restatement, for every (lane, cell, flag)."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SRC = r'''
#include "%s/dynamont_amd/csrc/decision_record.hpp"
extern "C" {
int rec_cpl() { return dynrec::REC_CPL; }
int rec_bytes() { return dynrec::REC_BYTES; }
unsigned pack(int stored, unsigned decisions) {
  bool d[dynrec::REC_CPL];
  for (int j = 0; j < dynrec::REC_CPL; ++j) d[j] = (decisions >> j) & 1u;
  return dynrec::rec_pack(stored != 0, d);
}
int decision(unsigned byte, int j) { return dynrec::rec_decision(byte, j); }
int stored(unsigned byte) { return dynrec::rec_stored(byte); }
int slot_decision(const uint8_t* rec, int slot) { return dynrec::rec_slot_decision(rec, slot); }
int slot_stored(const uint8_t* rec, int slot) { return dynk::lpe_slot_stored(rec, slot); }
}
''' % ROOT

CPL, LANES = 7, 64
u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("decrec")
    src = d / "t.cpp"
    src.write_text(SRC)
    so = d / "libt.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
    L = C.CDLL(str(so))
    L.pack.restype = C.c_uint
    L.pack.argtypes = [C.c_int, C.c_uint]
    L.decision.argtypes = [C.c_uint, C.c_int]
    L.stored.argtypes = [C.c_uint]
    L.slot_decision.argtypes = [u8p, C.c_int]
    L.slot_stored.argtypes = [u8p, C.c_int]
    return L


def test_geometry(lib):
    assert lib.rec_cpl() == CPL and lib.rec_bytes() == LANES


def test_pack_and_unpack_every_byte(lib):
    """All 2 x 128 (flag, decisions) values: the byte is flag << 7 | decisions, it fits a byte, and it unpacks to what went in."""
    seen = set()
    for stored, dec in itertools.product((0, 1), range(1 << CPL)):
        b = lib.pack(stored, dec)
        assert b == (stored << 7) | dec
        assert b < 256
        seen.add(b)
        assert lib.stored(b) == stored
        for j in range(CPL):
            assert lib.decision(b, j) == (dec >> j) & 1
    assert len(seen) == 256


def test_round_trip_every_lane_cell_and_flag(lib):
    """One (lane, cell) decision set in an otherwise empty record, with the lane's flag off and on, and its complement: exactly
    that slot reads as set (cleared), and exactly the 7 slots of that lane read as stored."""
    for lane, j, stored in itertools.product(range(LANES), range(CPL), (0, 1)):
        for invert in (False, True):
            rec = np.zeros(LANES, dtype=np.uint8)
            for l in range(LANES):
                dec = (1 << j) if l == lane else 0
                st = stored if l == lane else 0
                if invert:
                    dec, st = dec ^ 0x7f, st ^ 1
                rec[l] = lib.pack(st, dec)
            p = rec.ctypes.data_as(u8p)
            for slot in range(LANES * CPL):
                hit = slot == lane * CPL + j
                assert lib.slot_decision(p, slot) == int(hit != invert), (lane, j, stored, invert, slot)
                own = slot // CPL == lane
                assert lib.slot_stored(p, slot) == int((stored == 1 and own) != invert), (lane, j, stored, invert, slot)


def test_lpe_slot_stored_against_a_restatement(lib):
    """Random records: lpe_slot_stored(rec, slot) is bit 7 of byte slot // 7, for all 448 slots, whatever the decision bits."""
    rng = np.random.default_rng(20261020)
    for _ in range(200):
        rec = rng.integers(0, 256, LANES, dtype=np.uint8)
        p = rec.ctypes.data_as(u8p)
        got = [lib.slot_stored(p, s) for s in range(LANES * CPL)]
        want = [int(rec[s // 7]) >> 7 for s in range(LANES * CPL)]
        assert got == want
        got_d = [lib.slot_decision(p, s) for s in range(LANES * CPL)]
        want_d = [(int(rec[s // 7]) >> (s % 7)) & 1 for s in range(LANES * CPL)]
        assert got_d == want_d
