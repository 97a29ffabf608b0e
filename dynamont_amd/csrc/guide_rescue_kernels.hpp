// guide_rescue_kernels.hpp -- the guide rescue (dyn_aligner_set_guide_rescue, guide_rescue.hip): an align(calc = 1) job runs the
// plain alignment of every read, takes every read's band margins against the diagonal band, and re-aligns inside a self-made
// guide (k_auto_guide, then the refining banded-lattice launch) ONLY the reads whose margin says the band decided the alignment.
// Everything between the plain alignment and the riders happens on the device, in stream order, without a host round trip:
//   launch_band_margin      the diagonal margins of every read (band_margin_kernels.hpp), right behind the traceback
//   launch_rescue_select    the per-read code, and the list of the descriptors to rescue with its length
//   launch_auto_guide       over the list (AutoGuideArgs::active)
//   launch_band_reads       the refining launch over the list (BandArgs::active), into a SECOND set of per-row path arrays,
//                           segment rows and per-read states: the plain answer is not touched while the rescue runs
//   launch_rescue_merge     a rescue that ended ok replaces the read's plain answer (code 1); one that failed is dropped (code 3)
// An empty list costs two launches whose workgroups end at their first queue read, and two small kernels.
//
// The per-read code (uint8): 0 not flagged (a read the plain alignment failed included), 1 rescued, 2 flagged but its lattice
// arena does not fit (T above max_T), 3 flagged but the rescue alignment failed; 2 and 3 keep the plain answer bit for bit.
//
// The decision rule is rescue_decide below, a host/device function: its g++ build is checked against a Python restatement
// (tests/test_guide_rescue_host.py).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DYN_RESCUE_HD __host__ __device__ inline
#else
#define DYN_RESCUE_HD inline
#endif

namespace dynk {

constexpr uint8_t RESCUE_NONE = 0, RESCUE_DONE = 1, RESCUE_NO_ROOM = 2, RESCUE_FAILED = 3;

// A read is flagged when its plain alignment is ok, it has a border at all (N >= 2) and the smaller of its two margins is below
// min_margin; a margin of 0xFFFFFFFF ("never a real edge") is the largest uint32 and so never below anything. Returns 0 (not
// flagged), 1 (flagged, to be rescued) or 2 (flagged, T above max_T: no arena holds its lattice).
DYN_RESCUE_HD uint8_t rescue_decide(int32_t status, uint32_t N, uint32_t T, uint32_t low, uint32_t high, uint32_t min_margin,
                                    uint32_t max_T) {
  if (status != 0 || N < 2) return 0;
  const uint32_t m = low < high ? low : high;
  if (!(m < min_margin)) return 0;
  return T <= max_T ? (uint8_t)1 : (uint8_t)2;
}

}  // namespace dynk

// ---- launch interface (DYN_GUIDE_RESCUE_RULE_ONLY: the rule above alone, for a plain host build without the HIP headers) ----
#if !defined(DYN_GUIDE_RESCUE_RULE_ONLY)
#include "nt_kernels.hpp"

namespace dynk {

struct RescueSelect {
  const ReadDesc* descs;   // the job's descriptor table in processing order
  int n_reads;
  const ReadState* st;     // the plain alignment's states
  const uint32_t* low;     // [reads of the batch] the diagonal margins launch_band_margin wrote
  const uint32_t* high;
  uint32_t min_margin;
  uint32_t max_T;          // the longest T whose lattice arena fits (0: none does)
  uint8_t* code;           // [reads of the batch] cleared by the caller; 1 (provisional: launch_rescue_merge decides) or 2 where flagged
  uint32_t* list;          // [n_reads] descriptor indices to rescue, ascending
  uint32_t* n_list;        // their number
};
// one workgroup walks the table in descriptor order and scans the flags: no atomics, the same list on every run
hipError_t launch_rescue_select(const RescueSelect& r, hipStream_t s);

struct RescueMerge {
  const ReadDesc* descs;
  int n_reads;
  const uint32_t* list;     // what launch_rescue_select wrote
  const uint32_t* n_list;
  const ReadState* st_in;   // the rescue's states, path arrays and segment rows ...
  const double* pp_in;
  const uint32_t* pathn_in;
  const uint32_t* segrow_in;
  ReadState* st;            // ... and the job's own, which hold the plain answer
  double* pp;
  uint32_t* pathn;
  uint32_t* segrow;
  uint8_t* code;            // [reads of the batch] 1 stays where the rescue ended ok, 3 where it did not
  uint32_t* rounds;         // [reads of the batch] of the listed reads: kept where code 1, cleared where code 3
  uint32_t* converged;
  int single;               // the rescue ran one alignment per read and no comparison (max_rounds 1): rounds = 1, converged = 0
};
// block k owns list[k] (grid n_reads: the list's length is known on the device only)
hipError_t launch_rescue_merge(const RescueMerge& r, hipStream_t s);

}  // namespace dynk
#endif
