// decision_record.hpp -- the 64-byte record the forward sweep leaves per lattice row (PagePool::bits), one BYTE per lane.
//
// Lane l of the wave owns band slots l * CPL .. l * CPL + CPL - 1 (blocked layout, nt_kernels.hpp); byte l of a row's record
// is that lane's:
//   bit j (j < CPL): the traceback decision of the lane's cell j, vE(t, n) == vM(t-1, n) + LPE(t, n)  (NT_aligner_api.cpp:448)
//   bit 7:           the lane's float LPE cells of this row were stored (lpe_liveness.hpp; in-place layout: always set)
// The forward sweep builds the byte in a register of its own lane -- the flag, then one compare and one add-with-carry per
// cell, highest cell first -- and the row's record is ONE byte store per lane, 64 contiguous bytes: no ballot is moved
// between lanes. The readers (traceback, mpost) test one bit per (row, slot).
// Shared by the HIP kernels and by a host-side test (tests/test_decision_record_host.py compiles it with g++).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DYN_DR_HD __host__ __device__ __forceinline__
#else
#define DYN_DR_HD inline
#endif

namespace dynrec {

constexpr int REC_CPL = 7;            // cells per lane (nt_kernels.hpp: CPL)
constexpr int REC_BYTES = 64;         // one byte per lane
constexpr unsigned REC_STORED = 0x80u;

// the byte of one lane: decisions[j] != 0 sets bit j. Written the way the sweep accumulates it: acc = 2 acc + decision,
// from the flag down to cell 0 (the compiler's v_cmp + v_addc pair per cell).
DYN_DR_HD unsigned rec_pack(bool stored, const bool (&decisions)[REC_CPL]) {
  unsigned acc = stored ? 1u : 0u;
  for (int j = REC_CPL - 1; j >= 0; --j) acc = (acc + acc) + (decisions[j] ? 1u : 0u);
  return acc;
}

DYN_DR_HD bool rec_decision(unsigned byte, int j) { return (byte >> j) & 1u; }
DYN_DR_HD bool rec_stored(unsigned byte) { return (byte & REC_STORED) != 0; }

// band slot s of a row (s = lane * CPL + j): its decision, and whether the sweep stored its float LPE
DYN_DR_HD bool rec_slot_decision(const uint8_t* rec, int slot) { return rec_decision(rec[slot / REC_CPL], slot % REC_CPL); }

}  // namespace dynrec

namespace dynk {

// whether the forward sweep stored the float LPE of band slot `slot` of the row whose record is `rec` (lpe_liveness.hpp)
DYN_DR_HD bool lpe_slot_stored(const uint8_t* rec, int slot) { return dynrec::rec_stored(rec[slot / dynrec::REC_CPL]); }

}  // namespace dynk
