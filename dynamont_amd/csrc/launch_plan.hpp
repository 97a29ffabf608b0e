// launch_plan.hpp -- the host-only rules of the launch path, each stated once, in plain C++ on plain values (no HIP header, no
// dyn_batch): enqueue_job (launch.cpp), session_choose / session_publish (session.cpp) and the guide pre-pass (dynamont_mi.cpp)
// call it, and tests/test_launch_plan_host.py compiles it with g++ against a restatement of every rule.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

namespace dynplan {

// what nt_kernels.hpp calls dynk::NO_PAGE, READ_STRICT, READ_STRICT_START, P and ROW_WORDS * 8 (launch.cpp asserts the equalities)
constexpr uint32_t NO_PAGE = 0xffffffffu, READ_STRICT = 1u, READ_STRICT_START = 2u;
constexpr uint32_t STRICT_ALL = 0xffffffffu;  // strict_rows of a read whose every row is certified
constexpr uint64_t BAND_SLOTS = 448, ROW_RECORD_BYTES = 64;
// bytes of one lattice row in the pool: bE 8 B per band slot and the row's 64-byte record, plus the float LPE (4 B per slot) where
// it is kept apart -- in place the posterior takes the backward value's slot
constexpr uint64_t row_sep = BAND_SLOTS * 12 + ROW_RECORD_BYTES, row_inp = BAND_SLOTS * 8 + ROW_RECORD_BYTES;

// Duration of a read of T rows in default rows; strict_rows > 0: certified backward sweep, forward sweep up to that row.
// Cost of a certified row relative to a default one (ISA instruction counts of the row loops, confirmed on the device:
// profiles/r04/strict_mode_cost.json): backward 1.3, forward 1.4; a read spends 0.4 / 0.6 of its time in the two sweeps.
inline uint64_t cost_rows(uint64_t T, uint32_t strict_rows) {
  if (!strict_rows) return T;
  const uint64_t fr = std::min<uint64_t>(T, strict_rows);
  return (T * 100 + T * 12 + fr * 24) / 100;  // 0.4 T x 1.3 + 0.6 (T + 0.4 fr) = T (1 + 0.12) + 0.24 fr
}

// Queue order: most expensive reads first, so that the tail of the launch is made of the cheapest ones; reads of equal cost keep
// their order. S_of(i) is read i's sample count, strict_rows[i] its certified rows.
template <class SOf>
void cost_order(std::vector<uint32_t>& order, SOf S_of, const uint32_t* strict_rows) {
  auto cost = [&](uint32_t i) { return cost_rows(S_of(i) + 1, strict_rows[i]); };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost(x) > cost(y); });
}

// Length order (longest first, stable): what the planner of a page-starved launch and the spread of a paged session start from.
template <class SOf>
void length_order(std::vector<uint32_t>& order, SOf S_of) {
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return S_of(x) > S_of(y); });
}

// The descriptor of read `read` (Desc = dynk::ReadDesc): everything but n_pages and a reserved first_page, which are the caller's.
template <class Desc>
Desc make_desc(uint32_t read, uint64_t S, uint64_t kc, uint64_t half_band, uint64_t sig_off, uint64_t par_off, uint64_t seg_off,
               uint64_t path_off, uint32_t strict_rows) {
  Desc d{};
  d.T = (uint32_t)(S + 1);
  d.N = (uint32_t)(kc + 1);
  d.bw = (uint32_t)std::min<uint64_t>(half_band, d.N / 2);
  d.read = read;
  d.ratio = (double)d.N / (double)d.T;
  d.sig_off = sig_off;
  d.par_off = par_off;
  d.seg_off = seg_off;
  d.path_off = path_off;
  d.first_page = NO_PAGE;
  d.flags = !strict_rows ? 0u : strict_rows == STRICT_ALL ? READ_STRICT : READ_STRICT_START;
  d.strict_rows = strict_rows;
  return d;
}

// pages of 2^log_r rows that hold lattice rows 0 .. T = S + 1 (the launch's lambda and the session's function were this one)
inline uint32_t pages_of(uint64_t S, int log_r) { return (uint32_t)((S + 2 + (1ull << log_r) - 1) >> log_r); }

// Pages that keep every wave slot busy: the n_slots largest lattices at once (with strict reads in the batch the queue is not in
// length order, hence the explicit selection). Reorders `pages`.
inline uint64_t pages_wanted(std::vector<uint32_t>& pages, size_t n_slots) {
  const size_t top = std::min(n_slots, pages.size());
  std::partial_sort(pages.begin(), pages.begin() + top, pages.end(), std::greater<uint32_t>());
  uint64_t w = 0;
  for (size_t k = 0; k < top; ++k) w += pages[k];
  return w;
}

// Posterior layout (nt_kernels.hip, forward_sweep): the separate float LPE array makes the forward sweep 17 % faster but costs 12
// instead of 8 bytes of HBM per band slot. When the pool cannot hold a separate-layout lattice for every wave slot, waves wait for
// pages; in place then, if the wider concurrency is worth more than the faster sweep. DYN_FORCE_LAYOUT=inplace (or anything
// else: separate) overrides the rule. Returns true for the separate layout.
inline bool choose_lpe_layout(uint64_t budget, uint64_t wanted, uint64_t page_rows) {
  const double c_sep = std::min(1.0, (double)budget / ((double)wanted * page_rows * row_sep + 1.0));
  const double c_inp = std::min(1.0, (double)budget / ((double)wanted * page_rows * row_inp + 1.0));
  bool separate = !(c_sep < 1.0 && c_inp * 0.92 > c_sep);
  if (const char* f = std::getenv("DYN_FORCE_LAYOUT")) separate = std::strcmp(f, "inplace") != 0;
  return separate;
}

}  // namespace dynplan
