// launch.cpp -- one CLASSIC launch per (merged) batch: the planner of page-starved queues (plan_queue), the spread order of
// paged sessions, enqueue_job (read descriptors, lattice pool, k_read_queue, the banded-lattice kernel, the per-segment
// kernels -- everything enqueued on the compute stream without a host synchronisation) and collect_timing. Reference counterpart:
// the body of NTAligner::align / train (NT_aligner_api.cpp:230-312, 567-639) for one read at a time.
#include "engine_internal.hpp"
#include "band_reads.hpp"
#include "dp_math_strict.hpp"
#include "guided_band_kernels.hpp"
#include "auto_guide_kernels.hpp"
#include "guide_rescue_kernels.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <queue>

using dynhost::PoreModel;
using dynk::ReadDesc;
using dynk::ReadState;
using dynk::SegRow;
using dynmath::Emis;
using namespace dyneng;

namespace dyneng {

// ---- queue planning for page-starved launches ---------------------------------------------------
// The persistent waves take reads off the queue in order; a wave keeps its arena and exchanges pages with
// the pool only when its next read needs more (it then waits with no pages until the pool can serve it)
// or much less while somebody waits. Every wave sweeps rows at the same rate, so the whole launch can be
// replayed on the host: simulate_queue returns the makespan in rows for a given queue order.
static uint64_t simulate_queue(const std::vector<uint32_t>& need, const std::vector<uint64_t>& rows, size_t n_slots,
                               uint64_t pool) {
  const size_t n = need.size();
  struct Ev { uint64_t t; uint32_t slot; bool operator>(const Ev& o) const { return t > o.t; } };
  std::priority_queue<Ev, std::vector<Ev>, std::greater<Ev>> events;
  struct Wait { uint32_t slot, need; size_t idx; };
  std::vector<Wait> waiting;
  std::vector<uint32_t> have(n_slots, 0);
  uint64_t free_pages = pool, end = 0;
  size_t head = 0;
  auto serve = [&](uint64_t now) {
    for (size_t i = 0; i < waiting.size();) {
      if (free_pages >= waiting[i].need) {
        free_pages -= waiting[i].need;
        have[waiting[i].slot] = waiting[i].need;
        events.push(Ev{now + rows[waiting[i].idx], waiting[i].slot});
        waiting.erase(waiting.begin() + i);
      } else {
        ++i;
      }
    }
  };
  bool reserving = true;
  for (size_t s = 0; s < n_slots && s < n; ++s) {  // first round: pages reserved by the host while they last
    head = s + 1;
    if (reserving && free_pages >= need[s]) {
      free_pages -= need[s];
      have[s] = need[s];
      events.push(Ev{rows[s], (uint32_t)s});
    } else {
      reserving = false;
      waiting.push_back(Wait{(uint32_t)s, need[s], s});
    }
  }
  while (!events.empty()) {
    const Ev e = events.top();
    events.pop();
    end = std::max(end, e.t);
    uint32_t& hv = have[e.slot];
    if (head < n) {
      const size_t idx = head++;
      if (hv >= need[idx]) {
        if (!waiting.empty() && hv - need[idx] >= 8 && 8 * (hv - need[idx]) >= hv) {
          free_pages += hv - need[idx];
          hv = need[idx];
          serve(e.t);
        }
        events.push(Ev{e.t + rows[idx], e.slot});
      } else {
        free_pages += hv;
        hv = 0;
        waiting.push_back(Wait{e.slot, need[idx], idx});
        serve(e.t);
      }
    } else {
      free_pages += hv;
      hv = 0;
      serve(e.t);
    }
  }
  return waiting.empty() ? end : ~0ull;  // a plan that strands a read is no plan
}

// `order` comes in longest first. When the pool cannot hold a lattice for every wave slot, longest-first
// leaves the slots beyond the pool's capacity idle until the first long reads finish (config 3: 7.6 % of
// all wave time, measured). Candidate plans give those slots BRIDGE reads -- shorter reads whose arenas fit
// beside L long ones -- and start the displaced long reads when the first round's memory comes back:
//   queue = [ L longest | bridge = ranks [first, last), longest first | everything else, longest first ]
// The shortest quarter of the batch is never used as bridge (it keeps the launch's tail short). The plan
// with the smallest simulated makespan wins; plain longest-first is one of the candidates.
void plan_queue(std::vector<uint32_t>& order, const std::vector<uint32_t>& need, const std::vector<uint64_t>& rows,
                       size_t n_slots, uint64_t pool) {
  const size_t n = order.size();
  std::vector<uint64_t> pre(n + 1, 0), rpre(n + 1, 0);
  for (size_t k = 0; k < n; ++k) {
    pre[k + 1] = pre[k] + need[k];
    rpre[k + 1] = rpre[k] + rows[k];
  }
  size_t L0 = 0;
  while (L0 < n_slots && pre[L0 + 1] <= pool) ++L0;
  if (L0 >= n_slots || L0 < 2) return;  // every slot gets its lattice (or nothing sensible to plan)
  const size_t lo_rank = n - n / 4;
  auto permute = [&](size_t L, size_t first, size_t last, std::vector<uint32_t>& nd, std::vector<uint64_t>& rw,
                     std::vector<uint32_t>* ord) {
    nd.clear();
    rw.clear();
    if (ord) ord->clear();
    auto put = [&](size_t lo, size_t hi) {
      for (size_t k = lo; k < hi; ++k) {
        nd.push_back(need[k]);
        rw.push_back(rows[k]);
        if (ord) ord->push_back(order[k]);
      }
    };
    put(0, L);
    put(first, last);
    put(L, first);
    put(last, n);
  };
  std::vector<uint32_t> nd;
  std::vector<uint64_t> rw;
  uint64_t best = simulate_queue(need, rows, n_slots, pool);
  size_t bL = 0, bfirst = 0, blast = 0;
  const size_t step = std::max<size_t>(1, n_slots / 32);
  for (size_t L = L0; L + step > step && L >= n_slots / 4; L -= step) {
    const uint64_t per_slot = (pool - pre[L]) / (n_slots - L);
    size_t first = std::lower_bound(need.begin() + L, need.begin() + lo_rank, per_slot,
                                    [](uint32_t a, uint64_t v) { return a > v; }) - need.begin();  // first rank that fits
    if (lo_rank - first < n_slots - L) continue;
    const uint64_t target = (uint64_t)(n_slots - L) * rows[L - 1];
    for (int f = 2; f <= 6; ++f) {  // bridge rows = 0.5 .. 1.5 x "one long read per bridge slot"
      size_t last = std::lower_bound(rpre.begin() + first, rpre.begin() + lo_rank, rpre[first] + target * f / 4) - rpre.begin();
      last = std::min(std::max(last, first + (n_slots - L)), lo_rank);
      permute(L, first, last, nd, rw, nullptr);
      const uint64_t t = simulate_queue(nd, rw, n_slots, pool);
      if (t < best) {
        best = t;
        bL = L;
        bfirst = first;
        blast = last;
      }
    }
  }
  if (bL) {
    std::vector<uint32_t> planned;
    permute(bL, bfirst, blast, nd, rw, &planned);
    order.swap(planned);
  }
}

}  // namespace dyneng

namespace dyneng {
// SPREAD (paged sessions; `order` comes in longest first): in a stream of tickets the waves never start together, so what
// matters is that any ~n_waves consecutive reads ask for about the AVERAGE number of pages (config 3: 205 GB against a 250 GB
// pool) instead of the maximum (370 GB for the 1 024 longest). The longer (tail_div - 1) / tail_div of the reads are dealt out
// in a low-discrepancy order (rank k * phi mod m); the shortest 1 / tail_div follow, longest first, so that a ticket nobody
// follows still ends on short reads (tail_div 0: every read is spread). Config 3, same box: tail 1/8 507, 1/4 499-504, 1/2 493,
// none 509; the planned order (plan_queue) 465; one planned launch per batch 446-457 Msamp/s.
void spread_order(std::vector<uint32_t>& order, int tail_div) {
  const size_t n = order.size();
  const size_t m = tail_div > 0 ? n - n / (size_t)tail_div : n;
  if (m < 3) return;
  size_t step = (size_t)((double)m * 0.6180339887498949) | 1;
  auto gcd = [](size_t x, size_t y) { while (y) { const size_t t = x % y; x = y; y = t; } return x; };
  while (gcd(step, m) != 1) step += 2;
  std::vector<uint32_t> spread(order);
  for (size_t k = 0; k < m; ++k) spread[k] = order[(k * step) % m];
  order.swap(spread);
}
}  // namespace dyneng

extern "C" int dyn_session_order(uint64_t n_reads, uint32_t* order_out) {
  if (!order_out) return DYN_ERR_INVALID_ARGUMENT;
  std::vector<uint32_t> order(n_reads);
  for (uint64_t k = 0; k < n_reads; ++k) order[k] = (uint32_t)k;
  dyneng::spread_order(order, dyneng::SESSION_TAIL_DIV);
  if (n_reads) std::memcpy(order_out, order.data(), n_reads * sizeof(uint32_t));  // (an empty vector's data() may be null)
  return DYN_OK;
}

extern "C" int dyn_plan_queue(uint64_t n_reads, const uint32_t* pages, const uint64_t* rows, uint64_t n_slots,
                              uint64_t pool_pages, uint32_t* order_out, uint64_t* makespan_longest_first,
                              uint64_t* makespan_planned) {
  if (!pages || !rows || !order_out || !n_slots) return DYN_ERR_INVALID_ARGUMENT;
  std::vector<uint32_t> need(pages, pages + n_reads), order(n_reads);
  std::vector<uint64_t> rw(rows, rows + n_reads);
  for (uint64_t k = 0; k < n_reads; ++k) {
    order[k] = (uint32_t)k;
    if (k && need[k] > need[k - 1]) return DYN_ERR_INVALID_ARGUMENT;  // longest first
  }
  if (makespan_longest_first) *makespan_longest_first = dyneng::simulate_queue(need, rw, n_slots, pool_pages);
  if (n_reads > n_slots) dyneng::plan_queue(order, need, rw, n_slots, pool_pages);
  if (makespan_planned) {
    std::vector<uint32_t> nd(n_reads);
    std::vector<uint64_t> r2(n_reads);
    for (uint64_t k = 0; k < n_reads; ++k) {
      nd[k] = need[order[k]];
      r2[k] = rw[order[k]];
    }
    *makespan_planned = dyneng::simulate_queue(nd, r2, n_slots, pool_pages);
  }
  std::memcpy(order_out, order.data(), n_reads * sizeof(uint32_t));
  return DYN_OK;
}

namespace dyneng {

// Shared engine of align / train. Every ok read of the batch goes, longest first, into ONE launch of
// persistent waves (k_read_queue): a wave runs a read's whole pipeline and then takes the next read
// off the queue. The lattice of a read lives in pages of a pool that only has to hold the reads in
// flight (at most 4 per CU); the pages of the first round are reserved here, later reads take theirs
// from the pool's free list on the device. Everything is ENQUEUED on the handle's compute stream
// without a host synchronisation; host-side inputs of the launches (read descriptors, initial
// per-read state) live in pinned per-batch buffers until the batch is destroyed.
int enqueue_job(dyn_batch* b, DynJob job) {
  dyn_aligner* a = b->a;
  const bool lattice = job != DynJob::AlignZ;
  const bool calc = job == DynJob::AlignFull;
  const PoreModel& m = a->model;
  const int z_fail = job == DynJob::Train ? DYN_READ_TRAIN_Z_MISMATCH : DYN_READ_Z_MISMATCH;
  const int band_job = job == DynJob::Train ? 2 : calc ? 1 : 0;  // launch_band_reads' job
  const uint32_t refine_rounds = (b->guided && calc) ? b->guide_refine : 1;  // dyn_batch_set_guide_refine
  b->gref_ready = false;
  // the guide rescue (dyn_aligner_set_guide_rescue): sampled per job by the caller; it concerns the unguided align job with
  // probabilities alone (the callers refuse the combinations with rescale / border confidence / a guide)
  const bool rescue = calc && b->want.rescue_hw > 0 && !b->guided && !a->ntk && b->want.rescale_iters == 0 && b->want.border_confidence == 0;
  b->gr_ready = false;

  // mode "resquiggle"/"ntk": what the reference's NTKAligner does in this snapshot, as observed with the compiled
  // reference (tests/golden/g11_ntk_messages.json): validateInput / sequenceToKmers errors first, then EVERY read fails
  // its Zf/Zb check (NTK_aligner_api.cpp:911-917), and train() is the base class's "not implemented" (aligner.cpp:38-44).
  // No kernel runs; the reads get the per-read status whose message is the reference's exception text.
  if (a->ntk && job == DynJob::Train) {
    a->last_error = "Training is not implemented for this aligner";
    return DYN_ERR_RUNTIME;
  }
  // one launch per batch on the compute stream: the lattice pool must not be in the hands of resident waves
  if (int rc = session_quiesce(a)) return rc;
  // Strict reads (align(calc=true) only; dyn_aligner_set_strict) take the sweeps whose every sum is certified to be the
  // reference's bit for bit (dp_math_strict.hpp). Mode 2: every read, every row. Mode 1 (the default): the reads that carry
  // a structural tie (tie_rows above) -- their backward sweep in full and their forward sweep up to the row in which the
  // last tied column pair has left the band: the Viterbi values of a row depend on forward values of earlier rows only,
  // so every decision up to that row is the reference's own; later decisions have the ordinary >= 1e-6 margins. Strict
  // reads run in the SAME launch as the others (a per-read flag, kernel variant k_read_queue<JOB, true>).
  // Queue order: most expensive reads first, so that the tail of the launch is made of the cheapest ones.
  // Cost of a certified row relative to a default one (ISA instruction counts of the row loops, confirmed on the device:
  // profiles/r04/strict_mode_cost.json): backward 1.3, forward 1.4; a read spends 0.4 / 0.6 of its time in the two sweeps.
  const int32_t* km = b->kmers();
  std::vector<uint32_t> strict_rows(b->n, 0);
  std::vector<uint32_t> order, wide;
  uint64_t n_strict = 0;
  for (uint64_t i = 0; i < b->n; ++i) {
    const HostRead& r = b->reads[i];
    if (r.status != DYN_READ_OK) continue;
    if (a->ntk) continue;  // no read reaches the device; its status is set below
    // the banded-lattice kernel (band_reads.hip): the reference's own arithmetic in every cell, no pages. A wide read takes it
    // inside the reference's band, and every read of a guided batch (dyn_batch_set_guide), whatever its N, inside its guide's
    // window (such a batch then has no read for the read queue)
    if (r.wide || b->guided) {
      wide.push_back((uint32_t)i);
      continue;
    }
    if (calc && a->strict_mode == 2) strict_rows[i] = 0xffffffffu;
    else if (calc && a->strict_mode == 1) strict_rows[i] = tie_rows(a->model, km + r.flat_off, r.kc, r.S);
    n_strict += strict_rows[i] != 0;
    order.push_back((uint32_t)i);
  }
  auto is_strict = [&](uint32_t i) { return strict_rows[i] != 0; };
  auto cost_rows_strict = [&](uint32_t i) -> uint64_t {
    const uint64_t T = b->reads[i].S + 1, fr = std::min<uint64_t>(T, strict_rows[i]);
    return (T * 100 + T * 12 + fr * 24) / 100;  // 0.4 T x 1.3 + 0.6 (T + 0.4 fr) = T (1 + 0.12) + 0.24 fr
  };
  auto cost_rows = [&](uint32_t i) { return is_strict(i) ? cost_rows_strict(i) : b->reads[i].S + 1; };
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cost_rows(x) > cost_rows(y); });

  if (calc) {
    HIP_TRY(a, b->d_segrow.ensure(std::max<uint64_t>(4, b->capacity * 4)));
    HIP_TRY(a, b->d_medhi.ensure(std::max<uint64_t>(8, b->capacity * 8)));
    HIP_TRY(a, b->d_medlo.ensure(std::max<uint64_t>(8, b->capacity * 8)));
  }
  if (job == DynJob::Train) {
    HIP_TRY(a, b->d_colw.ensure(std::max<uint64_t>(8, b->total_cols * 8)));
    HIP_TRY(a, b->d_cols1.ensure(std::max<uint64_t>(8, b->total_cols * 8)));
    HIP_TRY(a, b->d_cols2.ensure(std::max<uint64_t>(8, b->total_cols * 8)));
    HIP_TRY(a, b->d_trans.ensure(std::max<uint64_t>(16, b->n * 16)));
    // (the DEVICE-resident pooled statistics -- a radix sort and a segmented sum behind every training launch, 2.4 % of it --
    //  have one reader, dyn_batch_device_pooled for the multi-GPU all-reduce: they are computed when it asks, round 5)
    b->pooled_on_device = false;
  }

  // HBM budget for the page pool
  uint64_t budget = mem_budget_left(a);
  if (lattice) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
    // the handle's own pool and the pools destroyed handles have parked on this device are not "free", but they are
    // this launch's to use: without the parked share the budget of a second handle depended on the process's history
    const uint64_t pool = a->ws.bytes + a->lpe.bytes + a->bits.bytes + parked_bytes(a->device);
    const uint64_t avail = (uint64_t)((double)(free_b + pool) * 0.90);
    if (budget == 0 || budget > avail) budget = avail;
  }

  // rows per page: the longest read must fit the waves' PT_MAX-entry page tables
  uint32_t max_T = 0;
  for (uint32_t i : order) max_T = std::max<uint32_t>(max_T, (uint32_t)(b->reads[i].S + 1));
  int log_r = dyneng::min_page_log_rows();
  while (((uint64_t)max_T + 1 + ((1ull << log_r) - 1)) >> log_r > (uint64_t)dynk::PT_MAX) ++log_r;
  const uint64_t page_rows = 1ull << log_r;
  auto pages_of = [&](uint64_t S) { return (uint32_t)((S + 2 + page_rows - 1) >> log_r); };  // rows 0 .. T = S+1
  const size_t n_slots = std::min<size_t>(order.size(), (size_t)a->n_cus * dynk::WAVES_PER_CU);
  // pages that keep every wave slot busy: the largest lattices at once (with strict reads in the batch the queue is
  // not in length order, hence the explicit selection)
  auto pages_wanted = [&]() {
    std::vector<uint32_t> pg(order.size());
    for (size_t k = 0; k < order.size(); ++k) pg[k] = pages_of(b->reads[order[k]].S);
    const size_t top = std::min(n_slots, pg.size());
    std::partial_sort(pg.begin(), pg.begin() + top, pg.end(), std::greater<uint32_t>());
    uint64_t w = 0;
    for (size_t k = 0; k < top; ++k) w += pg[k];
    return w;
  };
  uint64_t wanted = pages_wanted();

  // Posterior layout (nt_kernels.hip, forward_sweep): the separate float LPE array makes the forward sweep
  // 17 % faster but costs 12 instead of 8 bytes of HBM per band slot. When the pool cannot hold a
  // separate-layout lattice for every wave slot, waves wait for pages; in place then, if the wider
  // concurrency is worth more than the faster sweep.
  const uint64_t row_sep = (uint64_t)dynk::P * 12 + dynk::ROW_WORDS * 8, row_inp = (uint64_t)dynk::P * 8 + dynk::ROW_WORDS * 8;
  bool lpe_separate = calc;
  if (calc) {
    const double c_sep = std::min(1.0, (double)budget / ((double)wanted * page_rows * row_sep + 1.0));
    const double c_inp = std::min(1.0, (double)budget / ((double)wanted * page_rows * row_inp + 1.0));
    if (c_sep < 1.0 && c_inp * 0.92 > c_sep) lpe_separate = false;
    if (const char* f = std::getenv("DYN_FORCE_LAYOUT")) lpe_separate = std::string(f) != "inplace";
  }
  const uint64_t row_bytes = calc ? (lpe_separate ? row_sep : row_inp) : (uint64_t)dynk::P * 8;
  const uint64_t page_bytes = page_rows * row_bytes;

  // per-read state (status of host-side failures is final; ok reads start at 0). A read whose lattice
  // alone exceeds the budget fails on its own (the reference would die of std::bad_alloc for that read
  // only, segment.py:172-176), it does not take the batch with it.
  ReadState* st = b->h_state.as<ReadState>();
  for (uint64_t i = 0; i < b->n; ++i) {
    st[i].Zb = 0.0;
    st[i].Zf = 0.0;
    st[i].status = (a->ntk && b->reads[i].status == DYN_READ_OK) ? DYN_READ_NTK_MISMATCH : b->reads[i].status;
    st[i].n_segments = 0;
  }
  if (lattice) {
    size_t wr = 0;
    for (uint32_t i : order) {
      if ((uint64_t)pages_of(b->reads[i].S) * page_bytes > budget) st[i].status = DYN_READ_TOO_LARGE;
      else order[wr++] = i;
    }
    if (wr != order.size()) {
      order.resize(wr);
      wanted = pages_wanted();
    }
  }
  if (b->n) HIP_TRY(a, hipMemcpyAsync(b->d_state.p, st, b->n * sizeof(ReadState), hipMemcpyHostToDevice, a->stream));
  const size_t n_ok = order.size();

  // the pool: grow-only, shared by every batch of the handle (stream order serialises them)
  dynk::PagePool pool{};
  pool.log_rows = log_r;
  if (lattice && n_ok) {
    const uint64_t cap_pages = budget / page_bytes;
    const uint64_t target = std::min<uint64_t>(wanted, cap_pages);
    const uint64_t ws_pp = page_rows * dynk::P * 8, lpe_pp = page_rows * dynk::P * 4, bits_pp = page_rows * dynk::ROW_WORDS * 8;
    const bool grow = a->ws.bytes < target * ws_pp || (calc && lpe_separate && a->lpe.bytes < target * lpe_pp) ||
                      (calc && a->bits.bytes < target * bits_pp);
    if (grow) {  // growing releases the old buffer, which earlier work on the compute stream may still be using
      HIP_TRY(a, hipStreamSynchronize(a->stream));
      const double headroom = std::min(1.15, std::max(1.0, (double)cap_pages / (double)std::max<uint64_t>(1, target)));
      HIP_TRY(a, ensure_pool(a->device, a->ws, target * ws_pp, a->lpe, (calc && lpe_separate) ? target * lpe_pp : 0, a->bits,
                             calc ? target * bits_pp : 0, headroom));
    }
    uint64_t n_pages = std::min<uint64_t>(a->ws.bytes / ws_pp, cap_pages);  // (a buffer taken over from a parked pool may exceed this handle's budget)
    if (calc && lpe_separate) n_pages = std::min<uint64_t>(n_pages, a->lpe.bytes / lpe_pp);
    if (calc) n_pages = std::min<uint64_t>(n_pages, a->bits.bytes / bits_pp);
    n_pages = std::min<uint64_t>(n_pages, 0xfffffff0ull >> log_r);  // pool rows are 32-bit
    if (a->free_list.bytes < n_pages * 4) {
      HIP_TRY(a, hipStreamSynchronize(a->stream));
      HIP_TRY(a, a->free_list.ensure(n_pages * 4, 1.0));
    }
    pool.ws = a->ws.as<double>();
    pool.lpe = (calc && lpe_separate) ? a->lpe.as<float>() : nullptr;
    pool.bits = calc ? a->bits.as<uint64_t>() : nullptr;
    pool.free_list = a->free_list.as<uint32_t>();
    pool.n_pages = (uint32_t)n_pages;
  }
  HIP_TRY(a, a->ctl.ensure(dynk::QUEUE_CTL_WORDS * 4, 1.0));
  pool.ctl = a->ctl.as<uint32_t>();

  // Page-starved launches: the queue order is planned (plan_queue above); `rows` is each read's duration. The planner
  // works on a queue in LENGTH order (pages descending). A launch with strict reads is in cost order: when its first
  // round does not fit the pool it goes back to length order first -- a strict read costs 1.2x a plain one of its length,
  // which matters far less than idle slots in a starved launch (config 3 holds ~50 tie reads in 4 096; round 4's first
  // builds skipped the planner for such launches).
  if (lattice && order.size() > n_slots && !std::getenv("DYN_NO_BRIDGE")) {
    bool plan = true;
    if (n_strict) {
      uint64_t first_round = 0;
      for (size_t k = 0; k < n_slots; ++k) first_round += pages_of(b->reads[order[k]].S);
      plan = first_round > pool.n_pages;
      if (plan)
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return b->reads[x].S > b->reads[y].S; });
    }
    if (plan) {
      std::vector<uint32_t> need(order.size());
      std::vector<uint64_t> rows(order.size());
      for (size_t k = 0; k < order.size(); ++k) {
        need[k] = pages_of(b->reads[order[k]].S);
        rows[k] = cost_rows(order[k]);
      }
      plan_queue(order, need, rows, n_slots, pool.n_pages);
    }
  }

  // (Dealing the first round's strict reads out across the CUs instead of four to a CU was measured: 50.6 vs 50.9 ms on
  //  cfg2 with 26 % tie reads -- the certified sweeps do not get in each other's way inside a CU. Not kept.)

  // read descriptors in processing order; pages of the first round reserved here
  HIP_TRY(a, b->h_descs.ensure(std::max<size_t>(sizeof(ReadDesc), (n_ok + wide.size()) * sizeof(ReadDesc))));
  ReadDesc* descs = b->h_descs.as<ReadDesc>();
  dyn_timing tm{};
  uint64_t rows_total = 0;
  uint32_t used_pages = 0, n_static = 0, max_N = 0;
  bool reserving = true;
  for (size_t k = 0; k < order.size(); ++k) {
    const uint32_t i = order[k];
    const HostRead& r = b->reads[i];
    ReadDesc d{};
    d.T = (uint32_t)(r.S + 1);
    d.N = (uint32_t)(r.kc + 1);
    d.bw = (uint32_t)std::min<uint64_t>(m.half_band, d.N / 2);
    d.read = i;
    d.ratio = (double)d.N / (double)d.T;
    d.sig_off = r.sig_off;
    d.par_off = r.flat_off;
    d.seg_off = r.seg_off;
    d.path_off = rows_total;
    d.n_pages = lattice ? pages_of(r.S) : 0;
    d.first_page = dynk::NO_PAGE;
    d.flags = !is_strict(i) ? 0u : strict_rows[i] == 0xffffffffu ? dynk::READ_STRICT : dynk::READ_STRICT_START;
    d.strict_rows = strict_rows[i];
    if (reserving && k < n_slots && (!lattice || (uint64_t)used_pages + d.n_pages <= pool.n_pages)) {
      d.first_page = lattice ? used_pages : 0;
      used_pages += d.n_pages;
      n_static = (uint32_t)(k + 1);
    } else {
      reserving = false;  // later reads get their pages on the device
    }
    rows_total += d.T;
    max_N = std::max(max_N, d.N);
    descs[k] = d;
    tm.cells += (uint64_t)d.T * std::min<uint64_t>(2ull * d.bw + 1, d.N);
    tm.samples += r.S;
  }
  // the reads of the banded-lattice kernel: their descriptors FOLLOW the queue's (the read queue sees the first n_ok, the
  // per-segment kernels all). One lattice arena per workgroup, sized for the largest of them (none for Z only)
  uint64_t wide_arena = 0;
  int wide_groups = 0;
  // The arenas are the batch's own -- except a self-guided TICKET's (dyn_aligner_set_auto_guide), which uses the handle's: a
  // stream keeps many tickets in flight, each would hold workgroups x its largest lattice until the caller lets go of it (eight
  // tickets of 1 024 reads of 20 k samples at half width 64: 67 GB each), and only the ticket the compute stream is working on
  // needs them. Stream order hands the handle's arenas from one ticket to the next.
  dyneng::DevBuf& arena_buf = (b->async && b->guided) ? a->band_arena : b->d_arena;
  if (!wide.empty()) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
    uint64_t room = (uint64_t)((double)(free_b + arena_buf.bytes + parked_bytes(a->device)) * 0.8);
    if (b->guided && a->mem_budget && room > mem_budget_left(a)) room = mem_budget_left(a);
    size_t wr = 0;
    for (uint32_t i : wide) {
      const HostRead& r = b->reads[i];
      const uint64_t need = dynk::band_arena_bytes(r.S + 1, b->guided ? b->guide_hw : std::min<uint64_t>(m.half_band, (r.kc + 1) / 2), band_job);
      if (need > room) st[i].status = DYN_READ_TOO_LARGE;
      else {
        wide_arena = std::max(wide_arena, need);
        wide[wr++] = i;
      }
    }
    if (wr != wide.size()) {
      wide.resize(wr);
      if (b->n) HIP_TRY(a, hipMemcpyAsync(b->d_state.p, st, b->n * sizeof(ReadState), hipMemcpyHostToDevice, a->stream));
    }
    if (!wide.empty())
      wide_groups = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)wide.size(), (uint64_t)a->n_cus * (uint64_t)dynk::band_groups_per_cu(b->guided, (int)b->guide_hw, band_job),
                                                                   wide_arena ? room / wide_arena : ~0ull}));
  }
  b->arena_bytes = 0;
  const size_t n_all = n_ok + wide.size();
  for (size_t k = 0; k < wide.size(); ++k) {
    const uint32_t i = wide[k];
    const HostRead& r = b->reads[i];
    ReadDesc d{};
    d.T = (uint32_t)(r.S + 1);
    d.N = (uint32_t)(r.kc + 1);
    d.bw = (uint32_t)std::min<uint64_t>(m.half_band, d.N / 2);
    d.read = i;
    d.ratio = (double)d.N / (double)d.T;
    d.sig_off = r.sig_off;
    d.par_off = r.flat_off;
    d.seg_off = r.seg_off;
    d.path_off = rows_total;
    d.first_page = dynk::NO_PAGE;
    rows_total += d.T;
    max_N = std::max(max_N, d.N);
    descs[n_ok + k] = d;
    tm.cells += b->guided ? (uint64_t)d.T * (2ull * b->guide_hw + 1) : (uint64_t)d.T * std::min<uint64_t>(2ull * d.bw + 1, d.N);
    tm.samples += r.S;
  }
  if (calc) {
    HIP_TRY(a, b->d_pp.ensure(std::max<uint64_t>(8, rows_total * 8)));
    HIP_TRY(a, b->d_pathn.ensure(std::max<uint64_t>(4, rows_total * 4)));
  }
  HIP_TRY(a, b->d_descs.ensure(std::max<size_t>(sizeof(ReadDesc), n_all * sizeof(ReadDesc))));
  if (n_all)
    HIP_TRY(a, hipMemcpyAsync(b->d_descs.p, descs, n_all * sizeof(ReadDesc), hipMemcpyHostToDevice, a->stream));
  // ---- the guide rescue: what its stage needs is sized HERE, before anyone knows which reads will be flagged ----
  // One lattice arena per workgroup of the refining launch, sized for T_fit: the longest ok read for which at least one arena fits
  // what the page pool (allocated above) has left, within the handle's budget. A flagged read above T_fit gets code 2 on the
  // device. A ticket's arenas are the handle's, handed from ticket to ticket in stream order (as a self-guided ticket's are, and
  // for its reason); a synchronous batch's are the batch's own, shared with its wide reads' launch, which has ended by then.
  dyneng::DevBuf& resc_arena_buf = b->async ? a->band_arena : b->d_arena;
  uint64_t resc_arena = 0, resc_want = 0;
  uint32_t resc_T_fit = 0;
  int resc_groups = 0;
  if (rescue && n_all) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
    uint64_t room = (uint64_t)((double)(free_b + resc_arena_buf.bytes + parked_bytes(a->device)) * 0.8);
    if (a->mem_budget && room > mem_budget_left(a)) room = mem_budget_left(a);
    for (size_t k = 0; k < n_all; ++k)
      if (descs[k].T > resc_T_fit && dynk::band_arena_bytes(descs[k].T, b->want.rescue_hw, 1) <= room) resc_T_fit = descs[k].T;
    if (resc_T_fit) {
      resc_arena = dynk::band_arena_bytes(resc_T_fit, b->want.rescue_hw, 1);
      resc_groups = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)n_all, (uint64_t)a->n_cus * (uint64_t)dynk::band_groups_per_cu(true, (int)b->want.rescue_hw, 1),
                                                                    room / resc_arena}));
      resc_want = 256 + (uint64_t)resc_groups * resc_arena;
    }
  }
  // per-read rescaling (dyn_aligner_set_rescale): align(calc = 1) runs 1 + iters passes of everything below, in stream order
  const int iters = calc ? b->want.rescale_iters : 0;
  const int n_pass = 1 + iters;
  HIP_TRY(a, b->h_stats.ensure((size_t)n_pass * dynk::QUEUE_CTL_WORDS * 4));
  std::memset(b->h_stats.p, 0, (size_t)n_pass * dynk::QUEUE_CTL_WORDS * 4);
  // x0 is kept apart the first time a job of this batch rescales; every later job of the batch starts from it again
  uint64_t sig_len = 0;
  for (uint64_t i = 0; i < b->n; ++i) sig_len = std::max<uint64_t>(sig_len, b->reads[i].sig_off + b->reads[i].S);
  sig_len = std::min<uint64_t>(sig_len, b->d_sig.bytes / 8);
  if (b->sig0_kept) {
    if (b->sig0_len) HIP_TRY(a, hipMemcpyAsync(b->d_sig.p, b->d_sig0.p, b->sig0_len * 8, hipMemcpyDeviceToDevice, a->stream));
  } else if (iters) {
    HIP_TRY(a, b->d_sig0.ensure(std::max<uint64_t>(8, sig_len * 8)));
    if (sig_len) HIP_TRY(a, hipMemcpyAsync(b->d_sig0.p, b->d_sig.p, sig_len * 8, hipMemcpyDeviceToDevice, a->stream));
    b->sig0_kept = true;
    b->sig0_len = sig_len;
  }
  b->rs_ready = iters > 0;
  dynk::RescaleState* rs = nullptr;
  double* rs_y = nullptr;
  if (iters) {
    const uint64_t head = (b->n * sizeof(dynk::RescaleState) + 255) / 256 * 256;
    HIP_TRY(a, b->d_rs.ensure(std::max<uint64_t>(256, head + b->capacity * 8)));
    rs = b->d_rs.as<dynk::RescaleState>();
    rs_y = reinterpret_cast<double*>(b->d_rs.as<char>() + head);
    dynk::launch_rescale_init(rs, b->n, a->stream);
  }
  b->n_passes = n_pass;

  while (b->events.size() < 3) {
    hipEvent_t e = nullptr;
    HIP_TRY(a, hipEventCreate(&e));
    b->events.push_back(e);  // owned by the batch from here on: destroyed with it whatever happens next
  }
  hipEvent_t* ev = b->events.data();
  const int nr = (int)n_ok;
  dynk::QueueArgs q{};
  q.descs = b->d_descs.as<ReadDesc>();
  q.n_reads = nr;
  q.n_static = (int)n_static;
  q.sig = b->d_sig.as<double>();
  q.par = b->d_par.as<Emis>();
  q.pool = pool;
  q.st = b->d_state.as<ReadState>();
  q.tb = dynk::TraceBuffers{b->d_pp.as<double>(), b->d_pathn.as<uint32_t>(), b->d_segrow.as<uint32_t>(),
                            b->d_medhi.as<double>(), b->d_medlo.as<double>()};
  // (train jobs only: in an align job the posterior samples take their place, below)
  if (job == DynJob::Train) q.tr = dynk::TrainBuffers{b->d_colw.as<double>(), b->d_cols1.as<double>(), b->d_cols2.as<double>(), b->d_trans.as<double>()};
  q.m1 = m.log_m1;
  q.e2 = m.log_e2;
  q.sp_tab = a->d_sptab.as<dynmath::SoftplusNode>();
  q.z_fail_status = z_fail;
  q.lpe_floor = a->lpe_floor;
  q.lpe_dense = a->lpe_dense ? 1 : 0;
  // per-border posterior confidence: [border_probability | border_window_probability] x capacity, zeroed here (rows of reads
  // that fail keep the zeros), written by the read queue / the wide-band kernel of the LAST pass behind every read
  if (int rc = output_prepare(b, OUT_BORDERS, calc ? output_wanted(b->want, OUT_BORDERS) : 0, a->stream)) return rc;
  double* bc_cols = b->out[OUT_BORDERS].ready ? b->out[OUT_BORDERS].d.as<double>() : nullptr;
  // credible intervals: [mean | sd] f64 and [lo | hi] u32 x capacity in one buffer, zeroed here (rows of reads that fail keep the
  // zeros), written by the read queue / the banded-lattice kernel of the LAST pass behind every read
  if (int rc = output_prepare(b, OUT_INTERVALS, calc ? output_wanted(b->want, OUT_INTERVALS) : 0, a->stream)) return rc;
  const bool bi_on = b->out[OUT_INTERVALS].ready != 0;
  // soft levels: [weight | sum | sumsq] f64 x capacity in one buffer, zeroed here (rows of reads that fail keep the zeros), written
  // by the read queue / the banded-lattice kernel of the LAST pass behind every read
  if (int rc = output_prepare(b, OUT_SOFT, calc ? output_wanted(b->want, OUT_SOFT) : 0, a->stream)) return rc;
  const bool sl_on = b->out[OUT_SOFT].ready != 0;
  // posterior path samples: [count][capacity] segment starts, then the per-read count of dead samples, zeroed here (rows of reads
  // that fail keep the zeros), written by the read queue / the banded-lattice kernel behind every read. (The callers refuse the
  // switches that would make this more than one pass.)
  if (int rc = output_prepare(b, OUT_SAMPLES, calc ? output_wanted(b->want, OUT_SAMPLES) : 0, a->stream)) return rc;
  if (b->out[OUT_SAMPLES].ready) {
    q.sample.start = b->out[OUT_SAMPLES].d.as<uint32_t>();  // (the dead counts follow the planes)
    q.sample.capacity = b->capacity;
    q.sample.seed = b->want.sample_seed;
    q.sample.count = b->want.posterior_samples;
    q.lpe_dense = 1;  // a sampled path may visit any cell of the band (the kernel variant that carries the phase stores densely anyway)
  }
  const dynk::QueueJob qjob = job == DynJob::Train ? (a->train_zcheck ? dynk::JOB_TRAIN_ZCHECK : dynk::JOB_TRAIN)
                              : !calc              ? dynk::JOB_Z
                              : lpe_separate       ? dynk::JOB_ALIGN
                                                   : dynk::JOB_ALIGN_INPLACE;
  if (!b->ev_done) HIP_TRY(a, hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
  // The plan above (order, pages, strict rows) depends on T, N and the k-mers only: every pass reuses it. Each pass resets
  // what a launch resets -- per-read state, queue head and page pool (k_pool_init), the banded-lattice kernel's head (launch_band_reads).
  for (int pass = 0; pass < n_pass; ++pass) {
    if (pass > 0 && b->n) HIP_TRY(a, hipMemcpyAsync(b->d_state.p, st, b->n * sizeof(ReadState), hipMemcpyHostToDevice, a->stream));
    dynk::launch_pool_init(pool, used_pages, (int)n_static, a->stream);
    if (bc_cols && pass + 1 == n_pass) {
      q.border_window = b->want.border_confidence;
      q.lpe_dense = 1;  // the border phase reads whole windows of LPE (the kernel variant that carries it stores densely anyway)
      q.border_p = bc_cols;
      q.border_window_p = bc_cols + b->capacity;
    }
    if (bi_on && pass + 1 == n_pass) {  // (the callers refuse the border confidence and the samples beside it)
      q.interval = dynk::IntervalOut{b->out[OUT_INTERVALS].d.as<double>(), b->capacity, (1.0 - b->want.border_interval) / 2, 0};
      q.lpe_dense = 1;  // the phase reads whole columns of LPE (the kernel variant that carries it stores densely anyway)
    }
    if (sl_on && pass + 1 == n_pass) {  // (the callers refuse the other three lattice phases beside it)
      q.soft = dynk::SoftOut{b->out[OUT_SOFT].d.as<double>(), b->capacity, 0, dynk::SOFT_TAG};
      q.lpe_dense = 1;  // the phase reads whole columns of LPE (the kernel variant that carries it stores densely anyway)
    }
    if (pass == 0) HIP_TRY(a, hipEventRecord(ev[0], a->stream));
    dynk::launch_read_queue(qjob, n_strict != 0, q, a->n_cus, a->stream);
    if (pass + 1 == n_pass) HIP_TRY(a, hipEventRecord(ev[1], a->stream));
    // the statistics leave the control words before the next pass's or batch's k_pool_init resets them (same stream)
    HIP_TRY(a, hipMemcpyAsync(b->h_stats.as<uint32_t>() + (size_t)pass * dynk::QUEUE_CTL_WORDS, pool.ctl, dynk::QUEUE_CTL_WORDS * 4,
                              hipMemcpyDeviceToHost, a->stream));
    // (Running the per-segment kernels on a stream of their own, beside the next batch's read queue, was measured:
    //  the 0.35 ms gap it closes comes back as a 0.4 ms slower start of that read queue -- same-box A/B, no gain.)
    if (!wide.empty()) {
      // a queue of its own behind the read queue on the compute stream (its results feed the same per-segment kernels / the
      // same host finalisation)
      if (pass == 0) {
        // (a synchronous batch under the guide rescue: the rescue stage below works in the same buffer, which must not grow again)
        const uint64_t want = std::max<uint64_t>(256 + (uint64_t)wide_groups * wide_arena, &arena_buf == &resc_arena_buf ? resc_want : 0);
        size_t free_b = 0, total_b = 0;
        HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
        if (want > arena_buf.bytes && want > (uint64_t)((double)free_b * 0.95)) free_parked(a->device);  // (counted as room above)
        // (growing the handle's arenas releases the old ones, which the ticket before this one may still be working in)
        if (want > arena_buf.bytes && &arena_buf == &a->band_arena) HIP_TRY(a, hipStreamSynchronize(a->stream));
        HIP_TRY(a, arena_buf.ensure(want));
        b->arena_bytes = (uint64_t)wide_groups * wide_arena;
      }
      dynk::BandArgs ba{};
      ba.descs = q.descs + n_ok;
      ba.n_reads = (int)wide.size();
      ba.bw = (int)b->guide_hw;
      ba.sig = q.sig;
      ba.par = q.par;
      ba.guide = b->guided ? b->d_guide.as<int32_t>() : nullptr;  // null: the diagonal window
      ba.st = q.st;
      ba.tb = q.tb;
      ba.tr = q.tr;  // (an align job: the posterior samples, the credible intervals or the soft levels, which share the place)
      ba.head = arena_buf.as<uint32_t>();
      ba.arena = arena_buf.as<char>() + 256;
      ba.arena_bytes = wide_arena;
      ba.exp_tab = reinterpret_cast<const uint64_t*>(a->d_sptab.as<dynmath::SoftplusNode>() + dynmath::SP_NODES + dynmath::EXP128_NODES);
      ba.m1 = m.log_m1;
      ba.e2 = m.log_e2;
      ba.z_fail_status = z_fail;
      ba.border_window = q.border_window;  // (guided batches refuse the rider: dynamont_mi.cpp)
      ba.border_p = q.border_p;
      ba.border_window_p = q.border_window_p;
      // A TICKET that refines (dyn_aligner_set_auto_guide): ONE launch in which the workgroup that holds a read aligns it until
      // its guide reproduces itself (BandArgs::refine_rounds) -- a launch per round lasts as long as its longest read however
      // few reads are still open, which a stream of tickets cannot afford. The synchronous batch keeps the round scheme below:
      // it is what the refining launch is checked against, bit for bit.
      const bool refine_in_launch = refine_rounds > 1 && b->async;
      if (refine_in_launch) {
        HIP_TRY(a, b->d_gref.ensure(std::max<uint64_t>(8, 2 * b->n * 4)));
        HIP_TRY(a, hipMemsetAsync(b->d_gref.p, 0, 2 * b->n * 4, a->stream));
        ba.refine_rounds = (int)refine_rounds;
        ba.rounds = b->d_gref.as<uint32_t>();
        ba.converged = b->d_gref.as<uint32_t>() + b->n;
        b->gref_ready = true;
      }
      HIP_TRY(a, dynk::launch_band_reads(band_job, ba, wide_groups, a->stream));
      // guide refinement (dyn_batch_set_guide_refine): behind every alignment a step that makes the called path the next
      // guide of the reads whose guide it does not reproduce, and the list of those reads the next alignment's queue. Every
      // round is enqueued; a round whose list is empty ends at its first queue read. What follows the traceback
      // (launch_segments and the riders below) runs once, behind the last round
      if (refine_rounds > 1 && !refine_in_launch) {
        const uint64_t nb = b->n, nw = wide.size();
        HIP_TRY(a, b->d_gref.ensure((2 * nb + 64 + 2 * nw) * 4));
        uint32_t* g = b->d_gref.as<uint32_t>();
        HIP_TRY(a, hipMemsetAsync(g, 0, 2 * nb * 4, a->stream));
        uint32_t* cnt[2] = {g + 2 * nb, g + 2 * nb + 32};
        uint32_t* act[2] = {g + 2 * nb + 64, g + 2 * nb + 64 + nw};
        dynk::GuideRefine gr{};
        gr.descs = ba.descs;
        gr.n_reads = ba.n_reads;
        gr.st = q.st;
        gr.pathn = q.tb.pathn;
        gr.segrow = q.tb.segrow;
        gr.guide = b->d_guide.as<int32_t>();
        gr.rounds = g;
        gr.converged = g + nb;
        for (uint32_t r = 0; r < refine_rounds; ++r) {
          if (r > 0) {
            ba.active = act[(r - 1) & 1];
            ba.n_active = cnt[(r - 1) & 1];
            HIP_TRY(a, dynk::launch_band_reads(band_job, ba, wide_groups, a->stream));
          }
          gr.active_in = ba.active;
          gr.n_in = ba.n_active;
          gr.active_out = act[r & 1];
          gr.n_out = cnt[r & 1];
          gr.last = r + 1 == refine_rounds ? 1 : 0;
          HIP_TRY(a, dynk::launch_guide_refine(gr, a->stream));
        }
        b->gref_ready = true;
      }
    }
    // between two passes: the fit of every read and its signal recomputed from x0. (The per-segment kernels run once, after
    // the last pass: the fit reads the borders the traceback wrote, segrow, and nothing of k_median / k_final.)
    if (pass + 1 < n_pass)
      dynk::launch_rescale_pass(q.descs, (int)n_all, max_T, q.st, q.tb, b->d_sig0.as<double>(), b->d_sig.as<double>(), q.par, rs_y, rs, a->stream);
  }
  const int nr_all = (int)n_all;
  if (int rc = band_margin_prepare(b, calc != 0)) return rc;
  // ---- the guide rescue stage: behind the read queue and the diagonal banded-lattice launch, in front of the riders ----
  // (guide_rescue_kernels.hpp lists the launches). The host waits for none of them: a ticket's front thread enqueues the lot.
  if (rescue) {
    const uint64_t nb = b->n;
    const uint64_t off_code = 2 * nb * 4, off_len = (off_code + nb + 255) / 256 * 256, off_list = off_len + 256;
    const uint64_t off_bm = off_list + (uint64_t)n_all * 4;
    HIP_TRY(a, b->d_resc.ensure(std::max<uint64_t>(512, off_bm + (b->bm_ready ? 0 : 3 * nb * 4))));
    HIP_TRY(a, hipMemsetAsync(b->d_resc.p, 0, off_list, a->stream));  // rounds, converged, code, list length
    char* rb = b->d_resc.as<char>();
    uint32_t* g_rounds = reinterpret_cast<uint32_t*>(rb);
    uint32_t* g_conv = g_rounds + nb;
    uint8_t* g_code = reinterpret_cast<uint8_t*>(rb + off_code);
    uint32_t* g_len = reinterpret_cast<uint32_t*>(rb + off_len);
    uint32_t* g_list = reinterpret_cast<uint32_t*>(rb + off_list);
    // the diagonal margins of every read, whether or not the job reports margins: into the job's own arrays when it does
    uint32_t* marg = b->bm_ready ? b->d_bm.as<uint32_t>() : reinterpret_cast<uint32_t*>(rb + off_bm);
    const dynk::BandMargin dm{marg, marg + nb, marg + 2 * nb, 0u, (uint32_t)nb};
    dynk::launch_band_margin(q.descs, nr_all, max_N, q.st, q.tb, dm, a->stream);
    dynk::RescueSelect sel{};
    sel.descs = q.descs;
    sel.n_reads = nr_all;
    sel.st = q.st;
    sel.low = dm.low;
    sel.high = dm.high;
    sel.min_margin = b->want.rescue_margin;
    sel.max_T = resc_T_fit;
    sel.code = g_code;
    sel.list = g_list;
    sel.n_list = g_len;
    HIP_TRY(a, dynk::launch_rescue_select(sel, a->stream));
    if (resc_T_fit && nr_all) {
      // the guide (zero-filled, one int32 per sample of the batch) and the pre-pass's queue head behind it
      const uint64_t total = b->reads[b->n - 1].sig_off + b->reads[b->n - 1].S;
      const uint64_t head_off = (total * 4 + 255) / 256 * 256;
      HIP_TRY(a, b->d_guide.ensure(head_off + 256));
      if (total) HIP_TRY(a, hipMemsetAsync(b->d_guide.p, 0, total * 4, a->stream));
      dynk::AutoGuideArgs ag{};
      ag.descs = q.descs;
      ag.n_reads = nr_all;
      ag.bw = (int)b->want.rescue_hw;
      ag.sig = q.sig;
      ag.par = q.par;
      ag.guide = b->d_guide.as<int32_t>();
      ag.head = reinterpret_cast<uint32_t*>(b->d_guide.as<char>() + head_off);
      ag.m1 = m.log_m1;
      ag.e2 = m.log_e2;
      ag.active = g_list;
      ag.n_active = g_len;
      const int ag_groups = (int)std::min<uint64_t>(n_all, (uint64_t)a->n_cus * (uint64_t)dynk::auto_guide_groups_per_cu((int)b->want.rescue_hw));
      HIP_TRY(a, dynk::launch_auto_guide(ag, ag_groups, a->stream));
      // the rescue alignment writes a state, path rows and segment rows of its OWN (the read's offsets, other buffers): the
      // plain answer stays whole until launch_rescue_merge has seen how the rescue ended
      HIP_TRY(a, b->d_resc_st.ensure(std::max<uint64_t>(sizeof(ReadState), nb * sizeof(ReadState))));
      HIP_TRY(a, b->d_resc_pp.ensure(std::max<uint64_t>(8, rows_total * 8)));
      HIP_TRY(a, b->d_resc_pathn.ensure(std::max<uint64_t>(4, rows_total * 4)));
      HIP_TRY(a, b->d_resc_segrow.ensure(std::max<uint64_t>(4, b->capacity * 4)));
      {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
        if (resc_want > resc_arena_buf.bytes && resc_want > (uint64_t)((double)free_b * 0.95)) free_parked(a->device);  // (counted as room above)
        // (growing the handle's arenas releases the old ones, which the ticket before this one may still be working in)
        if (resc_want > resc_arena_buf.bytes && &resc_arena_buf == &a->band_arena) HIP_TRY(a, hipStreamSynchronize(a->stream));
        HIP_TRY(a, resc_arena_buf.ensure(resc_want));
        b->arena_bytes = std::max<uint64_t>(b->arena_bytes, resc_want - 256);
      }
      dynk::BandArgs ra{};
      ra.descs = q.descs;
      ra.n_reads = nr_all;
      ra.bw = (int)b->want.rescue_hw;
      ra.sig = q.sig;
      ra.par = q.par;
      ra.guide = b->d_guide.as<int32_t>();
      ra.st = b->d_resc_st.as<ReadState>();
      ra.tb = dynk::TraceBuffers{b->d_resc_pp.as<double>(), b->d_resc_pathn.as<uint32_t>(), b->d_resc_segrow.as<uint32_t>(), nullptr, nullptr};
      ra.head = resc_arena_buf.as<uint32_t>();
      ra.arena = resc_arena_buf.as<char>() + 256;
      ra.arena_bytes = resc_arena;
      ra.exp_tab = reinterpret_cast<const uint64_t*>(a->d_sptab.as<dynmath::SoftplusNode>() + dynmath::SP_NODES + dynmath::EXP128_NODES);
      ra.m1 = m.log_m1;
      ra.e2 = m.log_e2;
      ra.z_fail_status = z_fail;
      ra.active = g_list;
      ra.n_active = g_len;
      ra.refine_rounds = (int)b->want.rescue_rounds;
      ra.rounds = g_rounds;
      ra.converged = g_conv;
      HIP_TRY(a, dynk::launch_band_reads(1, ra, resc_groups, a->stream));
      dynk::RescueMerge mg{};
      mg.descs = q.descs;
      mg.n_reads = nr_all;
      mg.list = g_list;
      mg.n_list = g_len;
      mg.st_in = ra.st;
      mg.pp_in = ra.tb.pp;
      mg.pathn_in = ra.tb.pathn;
      mg.segrow_in = ra.tb.segrow;
      mg.st = q.st;
      mg.pp = q.tb.pp;
      mg.pathn = q.tb.pathn;
      mg.segrow = q.tb.segrow;
      mg.code = g_code;
      mg.rounds = g_rounds;
      mg.converged = g_conv;
      mg.single = b->want.rescue_rounds <= 1 ? 1 : 0;
      HIP_TRY(a, dynk::launch_rescue_merge(mg, a->stream));
      // a rescued read reports its margins against the window it was aligned in, every other read against the diagonal (above)
      if (b->bm_ready)
        dynk::launch_guided_band_margin(q.descs, nr_all, b->max_T, q.st, q.tb, b->d_guide.as<int32_t>(), (int)b->want.rescue_hw, dm, a->stream, g_code);
    }
    b->gr_ready = true;
  }
  dynk::EventCols evc{};
  if (int rc = output_prepare(b, OUT_LEVELS, calc ? output_wanted(b->want, OUT_LEVELS) : 0, a->stream)) return rc;
  if (b->out[OUT_LEVELS].ready) {  // [mean | stdev | median] x capacity
    double* e = b->out[OUT_LEVELS].d.as<double>();
    evc = dynk::EventCols{q.sig, e, e + b->capacity, e + 2 * b->capacity};
  }
  dynk::ScoreCols scc{};
  if (int rc = output_prepare(b, OUT_SCORES, calc ? output_wanted(b->want, OUT_SCORES) : 0, a->stream)) return rc;
  if (b->out[OUT_SCORES].ready) {  // [median_delta | mad_delta | homogeneity | scratch] x capacity
    double* e = b->out[OUT_SCORES].d.as<double>();
    scc = dynk::ScoreCols{q.sig, e, e + b->capacity, e + 2 * b->capacity, e + 3 * b->capacity, b->want.segment_scores};
  }
  if (calc) {
    // the per-k-mer summary (once per job, after the last pass: the signal of a rescaling job is its last pass's)
    const std::vector<dynk::KmerSummary> ks = kmer_summary_args(b);
    // the band margins (likewise once, from the last pass's borders)
    const std::vector<dynk::BandMargin> bm = band_margin_args(b);
    // (a guided batch's margins are taken against its own window: k_bmargin_guided below, not the diagonal's staircase kernel)
    dynk::launch_segments(q.descs, nr_all, rows_total, max_N, q.st, q.tb, b->d_rows.as<SegRow>(), m.k, a->stream, evc,
                          ks.empty() ? dynk::KmerSummary{} : ks[0], scc, (bm.empty() || b->guided || rescue) ? dynk::BandMargin{} : bm[0]);
    for (size_t k = 1; k < ks.size(); ++k) dynk::launch_kmer_summary(q.descs, nr_all, max_N, q.st, q.tb, ks[k], a->stream);
    // the per-site summary (likewise once: the last pass's signal, the borders the rescue left)
    enqueue_site_summary(b, q.descs, nr_all, max_N, q.st, q.tb, a->stream);
    // (under the guide rescue the margins were taken above, in front of the selection: such a job is never a merged launch)
    for (size_t k = b->guided ? 0 : 1; k < bm.size() && !rescue; ++k) {
      if (b->guided) dynk::launch_guided_band_margin(q.descs, nr_all, b->max_T, q.st, q.tb, b->d_guide.as<int32_t>(), (int)b->guide_hw, bm[k], a->stream);
      else dynk::launch_band_margin(q.descs, nr_all, max_N, q.st, q.tb, bm[k], a->stream);
    }
  }
  if (job == DynJob::Train) {
    b->pool_nr = nr_all;
    b->pool_max_N = max_N;
  }
  HIP_TRY(a, hipEventRecord(ev[2], a->stream));
  HIP_TRY(a, hipEventRecord(b->ev_done, a->stream));
  HIP_TRY(a, hipGetLastError());
  tm.reads_ok = n_all;
  tm.reads_strict = (uint32_t)n_strict;
  tm.launch_share = 1.0;
  b->strict_flag.assign(b->n, 0);
  for (uint64_t i = 0; i < b->n; ++i) b->strict_flag[i] = strict_rows[i] != 0;
  tm.launches = (nr || !wide.empty()) ? 1 : 0;
  tm.lp_inplace = (calc && !lpe_separate) ? 1 : 0;
  tm.pool_pages = pool.n_pages;
  tm.page_rows = (uint32_t)page_rows;
  tm.n_static = n_static;
  tm.n_waves = (uint32_t)std::min<size_t>((order.size() + dynk::WAVES_PER_CU - 1) / dynk::WAVES_PER_CU * dynk::WAVES_PER_CU,
                                         (size_t)a->n_cus * dynk::WAVES_PER_CU);
  b->timing = tm;
  b->n_chunks = (nr || !wide.empty()) ? 1 : 0;
  b->aligned = job != DynJob::Train;
  b->trained = job == DynJob::Train;
  b->last_calc = calc ? 1 : 0;
  return DYN_OK;
}

std::vector<dynk::KmerSummary> kmer_summary_args(const dyn_batch* b) {
  std::vector<dynk::KmerSummary> out;
  const dyn_aligner* a = b->a;
  if (!b->want.kmer_summary || !a->d_ksum.p) return out;
  unsigned long long* acc = a->d_ksum.as<unsigned long long>();
  dynk::KmerSummary ks{b->d_sig.as<double>(), b->d_kmers.as<int32_t>(), acc, acc + 6 * a->model.num_kmers,
                       (uint32_t)a->model.num_kmers, 0u, (uint32_t)b->n};
  if (b->ks_ranges.empty()) {
    out.push_back(ks);
  } else {
    for (const auto& r : b->ks_ranges) {
      ks.read_lo = r.first;
      ks.read_hi = r.second;
      out.push_back(ks);
    }
  }
  return out;
}

std::vector<dynk::SiteSummary> site_summary_args(const dyn_batch* b) {
  std::vector<dynk::SiteSummary> out;
  if (!b->want.site_summary || !b->ss_table || !b->ss_num_sites || !b->has_sites || !b->d_sites.p) return out;
  dynk::SiteSummary ss{b->d_sig.as<double>(), b->d_sites.as<uint32_t>(), b->ss_table, b->ss_table + (uint64_t)dynk::SS_FIELDS * b->ss_num_sites,
                       (uint32_t)b->ss_num_sites, 0u, (uint32_t)b->n};
  if (b->ss_ranges.empty()) {  // (a merged launch has ids only when a member that asked staged some: its ranges are never empty)
    out.push_back(ss);
  } else {
    for (const auto& r : b->ss_ranges) {
      ss.read_lo = r.first;
      ss.read_hi = r.second;
      out.push_back(ss);
    }
  }
  return out;
}

void enqueue_site_summary(const dyn_batch* b, const dynk::ReadDesc* descs, int n_reads, uint32_t max_N, const dynk::ReadState* st,
                          const dynk::TraceBuffers& tb, hipStream_t s) {
  for (const dynk::SiteSummary& ss : site_summary_args(b)) dynk::launch_site_summary(descs, n_reads, max_N, st, tb, ss, s);
}

int output_ensure(dyn_batch* b, Output k, int ready) {
  OutputBuf& o = b->out[k];
  o.ready = 0;
  if (!ready) return DYN_OK;
  const uint64_t bytes = (uint64_t)ready * OUTPUTS[k].row_bytes * b->capacity + (k == OUT_SAMPLES ? b->n * 4 : 0);
  HIP_TRY(b->a, o.d.ensure(std::max<uint64_t>(32, bytes)));
  o.ready = ready;
  return DYN_OK;
}

int output_zero(dyn_batch* b, Output k, hipStream_t s) {
  const uint64_t bytes = (uint64_t)b->out[k].ready * OUTPUTS[k].row_bytes * b->capacity + (k == OUT_SAMPLES ? b->n * 4 : 0);
  if (b->out[k].ready && bytes) HIP_TRY(b->a, hipMemsetAsync(b->out[k].d.p, 0, bytes, s));
  return DYN_OK;
}

int output_prepare(dyn_batch* b, Output k, int ready, hipStream_t s) {
  if (int rc = output_ensure(b, k, ready)) return rc;
  return output_zero(b, k, s);
}

int band_margin_prepare(dyn_batch* b, bool calc) {
  b->bm_ready = false;
  if (!calc || !b->want.band_margin) return DYN_OK;
  HIP_TRY(b->a, b->d_bm.ensure(std::max<uint64_t>(12, b->n * 12)));
  b->bm_ready = true;
  return DYN_OK;
}

std::vector<dynk::BandMargin> band_margin_args(const dyn_batch* b) {
  std::vector<dynk::BandMargin> out;
  if (!b->bm_ready || !b->n) return out;
  uint32_t* m = b->d_bm.as<uint32_t>();
  dynk::BandMargin bm{m, m + b->n, m + 2 * b->n, 0u, (uint32_t)b->n};
  if (b->bm_ranges.empty()) {
    out.push_back(bm);
  } else {
    for (const auto& r : b->bm_ranges) {
      bm.read_lo = r.first;
      bm.read_hi = r.second;
      out.push_back(bm);
    }
  }
  return out;
}

// After the compute stream has passed the batch (and the statistics copy behind it).
int collect_timing(dyn_batch* b) {
  dyn_aligner* a = b->a;
  dyn_timing& tm = b->timing;
  tm.ms_backward = tm.ms_forward = tm.ms_trace = tm.ms_total = tm.ms_dp = 0.0;
  tm.wave_wait_share = tm.wave_occupancy = 0.0;
  tm.ms_backward_strict = tm.ms_forward_strict = 0.0;
  tm.cert_fallbacks = tm.cert_rows = 0;
  if (!b->n_chunks) return DYN_OK;
  hipEvent_t* ev = b->events.data();
  float ms01 = 0, ms12 = 0;
  HIP_TRY(a, hipEventElapsedTime(&ms01, ev[0], ev[1]));
  HIP_TRY(a, hipEventElapsedTime(&ms12, ev[1], ev[2]));
  // wave-cycles per phase, summed over all waves of the launch: backward, forward, traceback (+ state
  // write-back and page release), waiting for a read / for pages, lifetime; [5] = longest lifetime
  // one record per pass (dyn_aligner_set_rescale): the cycle counts are summed, the longest lifetime is the longest of any
  uint64_t s[10] = {};
  for (int p = 0; p < b->n_passes; ++p) {
    const uint32_t* rec = b->h_stats.as<uint32_t>() + (size_t)p * dynk::QUEUE_CTL_WORDS;
    if (rec[3] != 0) {
      std::lock_guard<std::mutex> elk(a->err_mu);
      a->last_error = "the read queue aborted: a wave waited for the queue lock or for lattice pages for seconds";
      return DYN_ERR_DEVICE;
    }
    const uint64_t* sp = reinterpret_cast<const uint64_t*>(rec + dynk::QUEUE_STATS);
    for (int k = 0; k < 10; ++k) s[k] = k == 5 ? std::max(s[k], sp[k]) : s[k] + sp[k];
  }
  const double life = (double)s[4];
  tm.ms_dp = ms01;
  tm.ms_total = ms01 + ms12;
  if (life > 0) {
    tm.ms_backward = ms01 * (double)s[0] / life;
    tm.ms_forward = ms01 * (double)s[1] / life;
    tm.ms_trace = ms01 * (double)s[2] / life + ms12;
    tm.wave_wait_share = (double)s[3] / life;
    tm.ms_backward_strict = ms01 * (double)s[6] / life;
    tm.ms_forward_strict = ms01 * (double)s[7] / life;
    tm.cert_fallbacks = s[8];
    tm.cert_rows = s[9];
    if (s[5] && tm.n_waves) tm.wave_occupancy = life / ((double)s[5] * tm.n_waves);
  } else {
    tm.ms_trace = ms12;
  }
  return DYN_OK;
}

}  // namespace dyneng
