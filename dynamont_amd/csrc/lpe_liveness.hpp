// lpe_liveness.hpp -- which float LPE cells of a lattice row the forward sweep stores (separate posterior layout).
//
// The two readers of a stored LPE -- traceback (pp = exp((double)LPE)) and mpost (LPM rebuilt from LPE of the diagonal
// predecessor, pp = exp(LPM)) -- end in an fp64 exp, which is exactly 0 below about -745.14. A cell with LPE < floor
// (-750 by default) gives pp == 0.0 whether its float was stored or not, and so does the M cell mpost derives from it:
// bE(row-1, n-1) is a logPlus whose move operand is (bM(row, n) + e(row, n)) + m1, hence LPM(row, n) <= LPE(row-1, n-1)
// up to ~1e-11 of rounding; the float rounding of LPE adds <= 5e-5, and -750 lies 4.9 below the underflow point.
// So the readers substitute -inf for a cell that was not stored and the outputs keep every bit.
//
//   * a LANE is live when any of its CPL cells has !(LPE < floor): NaN is live (exp(NaN) is not 0; the lane's maximum is
//     taken with v_maximum3_f32, which hands a NaN on), and floor = -inf -- the dense switch -- makes every lane live, the
//     lanes outside the band included;
//   * a lane GROUP (LPE_GROUP = 16 lanes) is live when any of its lanes is, and all lanes of a live group store: the three
//     8-byte stores of a row then cover whole 128-byte runs and the 4-byte store a whole 64-byte one, never part of a sector
//     (8-lane groups would halve the 4-byte store's run; tools/ubench/stream_pattern.hip measures both patterns);
//   * every lane keeps its group's verdict as bit 7 of its byte of the row's record, above its CPL decision bits
//     (decision_record.hpp, which also holds the readers' lpe_slot_stored).
//
// tests/device_math/lpe_liveness.hip runs both functions on crafted rows against a host restatement.
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

#include "decision_record.hpp"

namespace dynk {

constexpr int LPE_GROUP = 16;             // lanes per store group
constexpr float LPE_STORE_FLOOR = -750.0f;

// IEEE-754-2019 maximum of three floats: NaN if any operand is NaN (v_max3_f32 would drop it). gfx950 has the instruction.
__device__ __forceinline__ float lpe_maximum3(float a, float b, float c) {
  float r;
  asm("v_maximum3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}

// a lane is live when any of its seven cells has !(f < floor): three f32 instructions and a compare, no fp64 work; a NaN
// cell makes the maximum NaN, and !(NaN < floor) holds
__device__ __forceinline__ bool lpe_lane_live(const float (&f)[7], float floor) {
  const float m = lpe_maximum3(lpe_maximum3(f[0], f[1], f[2]), lpe_maximum3(f[3], f[4], f[5]), f[6]);
  return !(m < floor);
}

// Whether this lane's group holds a live lane, as 0 / 1 in every lane. OR over each row of 16 lanes as a butterfly of four
// DPP steps (mirror the row, mirror its halves, swap neighbours, swap pairs): every lane of a row ends with the OR of all
// sixteen. It is bit 7 of the lane's byte of the row's record, and the seed of that byte's accumulator (decision_record.hpp).
__device__ __forceinline__ uint32_t lpe_store_flag(bool lane_live) {
  static_assert(LPE_GROUP == 16, "one DPP row");
  uint32_t x = lane_live ? 1u : 0u;
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xf, 0xf, true);  // row_mirror:           i <-> 15 - i
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xf, 0xf, true);  // row_half_mirror:      i <-> 7 - i in each half
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]:  i <-> i ^ 1
  x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xf, 0xf, true);   // quad_perm [2,3,0,1]:  i <-> i ^ 2
  return x;
}

// The lanes of the groups that hold a live lane, as a wave-uniform mask: the ballot of the flag IS the group mask (the exec
// mask of the row's LPE stores) and no scalar bit arithmetic follows.
__device__ __forceinline__ uint64_t lpe_store_mask(uint32_t flag) { return __ballot(flag != 0); }
__device__ __forceinline__ uint64_t lpe_store_mask(bool lane_live) { return lpe_store_mask(lpe_store_flag(lane_live)); }

}  // namespace dynk
