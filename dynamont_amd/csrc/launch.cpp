// launch.cpp -- one CLASSIC launch per (merged) batch: the planner of page-starved queues (plan_queue), the spread order of
// paged sessions, the steps the launch paths share (engine.hpp; their host-only rules: launch_plan.hpp), enqueue_job as a sequence of
// stages around a LaunchPlan (read descriptors, lattice pool, k_read_queue, the banded-lattice kernel, the per-segment kernels --
// everything enqueued on the compute stream without a host synchronisation) and collect_timing. Reference counterpart:
// the body of NTAligner::align / train (NT_aligner_api.cpp:230-312, 567-639) for one read at a time.
#include "engine_internal.hpp"
#include "launch_plan.hpp"
#include "band_reads.hpp"
#include "dp_math_strict.hpp"
#include "guided_band_kernels.hpp"
#include "auto_guide_kernels.hpp"
#include "guide_rescue_kernels.hpp"

#include <algorithm>
#include <cstring>
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

static_assert(dynplan::NO_PAGE == dynk::NO_PAGE && dynplan::READ_STRICT == dynk::READ_STRICT && dynplan::READ_STRICT_START == dynk::READ_STRICT_START &&
              dynplan::BAND_SLOTS == (uint64_t)dynk::P && dynplan::ROW_RECORD_BYTES == (uint64_t)dynk::ROW_WORDS * 8, "launch_plan.hpp restates nt_kernels.hpp");

// ---- what the classic launch, the resident session and the guide pre-pass share (engine.hpp) -------------------------------
// per-read state (status of host-side failures is final; ok reads start at 0)
ReadState* init_read_state(dyn_batch* b, bool ntk) {
  ReadState* st = b->h_state.as<ReadState>();
  for (uint64_t i = 0; i < b->n; ++i) {
    st[i].Zb = 0.0;
    st[i].Zf = 0.0;
    st[i].status = (ntk && b->reads[i].status == DYN_READ_OK) ? DYN_READ_NTK_MISMATCH : b->reads[i].status;
    st[i].n_segments = 0;
  }
  return st;
}

int arena_room(dyn_aligner* a, const DevBuf& buf, bool cap_by_budget, uint64_t* room) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
  *room = (uint64_t)((double)(free_b + buf.bytes + parked_bytes(a->device)) * 0.8);
  if (cap_by_budget && a->mem_budget && *room > mem_budget_left(a)) *room = mem_budget_left(a);
  return DYN_OK;
}

int grow_arena(dyn_aligner* a, DevBuf& buf, uint64_t want) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
  if (want > buf.bytes && want > (uint64_t)((double)free_b * 0.95)) free_parked(a->device);  // (counted as room by arena_room)
  // (growing the handle's arenas releases the old ones, which the ticket before this one may still be working in)
  if (want > buf.bytes && &buf == &a->band_arena) HIP_TRY(a, hipStreamSynchronize(a->stream));
  HIP_TRY(a, buf.ensure(want));
  return DYN_OK;
}

dynk::BandArgs band_args_common(const dyn_batch* b, const dynk::QueueArgs& q, int z_fail, const DevBuf& arena_buf, uint64_t arena_bytes) {
  const dyn_aligner* a = b->a;
  dynk::BandArgs ba{};
  ba.descs = q.descs;
  ba.sig = q.sig;
  ba.par = q.par;
  ba.st = q.st;
  ba.tb = q.tb;
  ba.head = arena_buf.as<uint32_t>();
  ba.arena = arena_buf.as<char>() + 256;
  ba.arena_bytes = arena_bytes;
  ba.exp_tab = reinterpret_cast<const uint64_t*>(a->d_sptab.as<dynmath::SoftplusNode>() + dynmath::SP_NODES + dynmath::EXP128_NODES);
  ba.m1 = a->model.log_m1;
  ba.e2 = a->model.log_e2;
  ba.z_fail_status = z_fail;
  return ba;
}

// one entry per range of reads whose ticket asked (a batch on its own has no ranges: the one entry that covers every read)
template <class Args>
static std::vector<Args> over_ranges(Args base, const std::vector<std::pair<uint32_t, uint32_t>>& ranges) {
  std::vector<Args> out;
  if (ranges.empty()) out.push_back(base);
  for (const auto& r : ranges) {
    base.read_lo = r.first;
    base.read_hi = r.second;
    out.push_back(base);
  }
  return out;
}

std::vector<dynk::KmerSummary> kmer_summary_args(const dyn_batch* b) {
  const dyn_aligner* a = b->a;
  if (!b->want.kmer_summary || !a->d_ksum.p) return {};
  unsigned long long* acc = a->d_ksum.as<unsigned long long>();
  const dynk::KmerSummary ks{b->d_sig.as<double>(), b->d_kmers.as<int32_t>(), acc, acc + 6 * a->model.num_kmers, (uint32_t)a->model.num_kmers, 0u, (uint32_t)b->n};
  return over_ranges(ks, b->ks_ranges);
}

std::vector<dynk::SiteSummary> site_summary_args(const dyn_batch* b) {
  if (!b->want.site_summary || !b->ss_table || !b->ss_num_sites || !b->has_sites || !b->d_sites.p) return {};
  // (a merged launch has ids only when a member that asked staged some: its ranges are never empty)
  // (a sparse table has ss_map.capacity rows, the totals behind them and the map's statistics behind the totals)
  const uint64_t rows = b->ss_map.keys ? b->ss_map.capacity : b->ss_num_sites;
  unsigned long long* totals = b->ss_table + (uint64_t)dynk::SS_FIELDS * rows;
  dynk::SiteSummary ss{b->d_sig.as<double>(), b->d_sites.as<uint32_t>(), b->ss_table, totals, (uint32_t)b->ss_num_sites, 0u, (uint32_t)b->n};
  if (b->ss_map.keys) {
    ss.map_keys = b->ss_map.keys;
    ss.capacity = (uint32_t)b->ss_map.capacity;
    ss.map_stats = totals + dynk::SS_TOTALS;
  }
  if (!b->want.site_histogram || !b->ss_hist.p) return over_ranges(ss, b->ss_ranges);
  // the histograms: a merged launch's members submitted with them on (sh_ranges) count, the others (ss_plain_ranges) add to the table alone
  std::vector<dynk::SiteSummary> out;
  if (!b->ss_plain_ranges.empty()) out = over_ranges(ss, b->ss_plain_ranges);
  ss.hist = b->ss_hist.p;
  ss.bins = b->ss_hist.bins;
  ss.hist_lo = b->ss_hist.lo;
  ss.inv_w = b->ss_hist.inv_w;
  for (const dynk::SiteSummary& x : over_ranges(ss, b->sh_ranges)) out.push_back(x);
  return out;
}

std::vector<dynk::SiteCalls> site_call_args(const dyn_batch* b) {
  if (!b->out[OUT_SITE_CALLS].ready || !b->n || !b->capacity) return {};
  const dyn_aligner* a = b->a;
  double* cols = b->out[OUT_SITE_CALLS].d.as<double>();  // [site_probability | site_z] x capacity
  dynk::SiteCalls sc{};
  sc.sig = b->d_sig.as<double>();
  sc.sites = (b->has_sites && b->d_sites.p) ? b->d_sites.as<uint32_t>() : nullptr;  // no ids staged: every row the NaN
  sc.model = b->ss_model;
  sc.map_keys = b->ss_map.keys;
  sc.capacity = (uint32_t)b->ss_map.capacity;
  sc.num_sites = (uint32_t)b->ss_num_sites;
  sc.read_lo = 0u;
  sc.read_hi = (uint32_t)b->n;
  sc.exp_tab = reinterpret_cast<const uint64_t*>(a->d_sptab.as<dynmath::SoftplusNode>() + dynmath::SP_NODES + dynmath::EXP128_NODES);
  sc.prob = cols;
  sc.z = cols + b->capacity;
  if (b->sc_ranges.empty()) return {sc};
  std::vector<dynk::SiteCalls> out;  // a merged launch: every member against the model it snapshot
  for (const dyn_batch::SiteCallRange& r : b->sc_ranges) {
    sc.read_lo = r.lo;
    sc.read_hi = r.hi;
    sc.model = r.model;
    if (!out.empty() && out.back().model == r.model && out.back().read_hi == r.lo) out.back().read_hi = r.hi;
    else out.push_back(sc);
  }
  return out;
}

std::vector<dynk::BandMargin> band_margin_args(const dyn_batch* b) {
  if (!b->bm_ready || !b->n) return {};
  uint32_t* m = b->d_bm.as<uint32_t>();
  return over_ranges(dynk::BandMargin{m, m + b->n, m + 2 * b->n, 0u, (uint32_t)b->n}, b->bm_ranges);
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

// The rider tail of an align(calc = 1) job, once behind its last pass (a rescaling job's last signal, the borders the rescue left):
// launch_segments with the columns, the first k-mer range and the first diagonal margin range; the other k-mer ranges; the site
// summary; the margins `margins` names. launch_site_summary and launch_band_margin read descs, st and segrow (the first sig and the
// site ids as well) and write tables of their own (the handle's site table; d_bm): their order is free, and is this one everywhere.
void enqueue_riders(dyn_batch* b, const ReadDesc* descs, int n, uint64_t rows_total, uint32_t max_N, const ReadState* st,
                   const dynk::TraceBuffers& tb, hipStream_t s, Margins margins) {
  const double* sig = b->d_sig.as<double>();
  dynk::EventCols evc{};
  if (b->out[OUT_LEVELS].ready) {  // [mean | stdev | median] x capacity
    double* e = b->out[OUT_LEVELS].d.as<double>();
    evc = dynk::EventCols{sig, e, e + b->capacity, e + 2 * b->capacity};
  }
  dynk::ScoreCols scc{};
  if (b->out[OUT_SCORES].ready) {  // [median_delta | mad_delta | homogeneity | scratch] x capacity
    double* e = b->out[OUT_SCORES].d.as<double>();
    scc = dynk::ScoreCols{sig, e, e + b->capacity, e + 2 * b->capacity, e + 3 * b->capacity, b->want.segment_scores};
  }
  const std::vector<dynk::KmerSummary> ks = kmer_summary_args(b);
  const std::vector<dynk::BandMargin> bm = band_margin_args(b);
  // (a guided batch's margins are taken against its own window: k_bmargin_guided below, not the diagonal's staircase kernel)
  dynk::launch_segments(descs, n, rows_total, max_N, st, tb, b->d_rows.as<SegRow>(), b->a->model.k, s, evc, ks.empty() ? dynk::KmerSummary{} : ks[0],
                        scc, (bm.empty() || margins != Margins::Diagonal) ? dynk::BandMargin{} : bm[0]);
  for (size_t k = 1; k < ks.size(); ++k) dynk::launch_kmer_summary(descs, n, max_N, st, tb, ks[k], s);
  for (const dynk::SiteSummary& ss : site_summary_args(b)) dynk::launch_site_summary(descs, n, max_N, st, tb, ss, s);
  // (behind the summary: a sparse map's buckets are only looked up here, and the model's ids have theirs since the upload)
  for (const dynk::SiteCalls& sc : site_call_args(b)) dynk::launch_site_calls(descs, n, max_N, st, tb, sc, s);
  if (margins == Margins::Diagonal)
    for (size_t k = 1; k < bm.size(); ++k) dynk::launch_band_margin(descs, n, max_N, st, tb, bm[k], s);
  if (margins == Margins::Guided)
    for (size_t k = 0; k < bm.size(); ++k)
      dynk::launch_guided_band_margin(descs, n, b->max_T, st, tb, b->d_guide.as<int32_t>(), (int)b->guide_hw, bm[k], s);
}

void record_job(dyn_batch* b, dyn_timing tm, DynJob job, bool calc, uint64_t reads_ok, uint64_t n_strict, const std::vector<uint32_t>& strict_rows, uint32_t n_chunks) {
  tm.reads_ok = reads_ok;
  tm.reads_strict = (uint32_t)n_strict;
  b->strict_flag.assign(b->n, 0);
  for (uint64_t i = 0; i < b->n; ++i) b->strict_flag[i] = strict_rows[i] != 0;
  b->timing = tm;
  b->n_chunks = n_chunks;
  b->aligned = job != DynJob::Train;
  b->trained = job == DynJob::Train;
  b->last_calc = calc ? 1 : 0;
}

// ---- enqueue_job, stage by stage ----------------------------------------------------------------------------------------------
// Shared engine of align / train. Every ok read of the batch goes, longest first, into ONE launch of
// persistent waves (k_read_queue): a wave runs a read's whole pipeline and then takes the next read
// off the queue. The lattice of a read lives in pages of a pool that only has to hold the reads in
// flight (at most 4 per CU); the pages of the first round are reserved here, later reads take theirs
// from the pool's free list on the device. Everything is ENQUEUED on the handle's compute stream
// without a host synchronisation; host-side inputs of the launches (read descriptors, initial
// per-read state) live in pinned per-batch buffers until the batch is destroyed.
namespace {

// What one stage of enqueue_job leaves for the later ones. The plan (order, pages, strict rows) depends on T, N and the k-mers
// only: every pass of a rescaling job reuses it.
struct LaunchPlan {
  DynJob job = DynJob::AlignFull;  // the job (enqueue_job)
  bool lattice = false, calc = false, rescue = false;
  int z_fail = 0, band_job = 0, n_pass = 1;
  uint32_t refine_rounds = 1;
  std::vector<uint32_t> order, wide, strict_rows;  // plan_reads: queue reads in processing order, the banded-lattice kernel's, certified rows per read
  uint64_t n_strict = 0;
  uint64_t budget = 0, page_rows = 0, page_bytes = 0;  // size_pool
  int log_r = 8;
  bool lpe_separate = false;
  dynk::QueueJob qjob = dynk::JOB_Z;
  size_t n_slots = 0, n_ok = 0;
  uint32_t max_T = 0;
  dynk::PagePool pool{};
  ReadState* st = nullptr;  // the batch's pinned initial state
  size_t n_all = 0;  // build_descs
  uint64_t rows_total = 0, wide_arena = 0;
  uint32_t used_pages = 0, n_static = 0, max_N = 0;
  int wide_groups = 0;
  DevBuf *arena_buf = nullptr, *resc_arena_buf = nullptr;  // (the second: size_rescue, as what follows)
  uint64_t resc_arena = 0, resc_want = 0;
  uint32_t resc_T_fit = 0;
  int resc_groups = 0;
  dynk::RescaleState* rs = nullptr;  // prepare_rescale
  double* rs_y = nullptr;
  dyn_timing tm{};

  uint32_t pages(const dyn_batch* b, uint32_t i) const { return dynplan::pages_of(b->reads[i].S, log_r); }  // rows 0 .. T = S+1
  uint64_t cost(const dyn_batch* b, uint32_t i) const { return dynplan::cost_rows(b->reads[i].S + 1, strict_rows[i]); }
};

// Strict reads (align(calc=true) only; dyn_aligner_set_strict) take the sweeps whose every sum is certified to be the
// reference's bit for bit (dp_math_strict.hpp). Mode 2: every read, every row. Mode 1 (the default): the reads that carry
// a structural tie (tie_rows) -- their backward sweep in full and their forward sweep up to the row in which the
// last tied column pair has left the band: the Viterbi values of a row depend on forward values of earlier rows only,
// so every decision up to that row is the reference's own; later decisions have the ordinary >= 1e-6 margins. Strict
// reads run in the SAME launch as the others (a per-read flag, kernel variant k_read_queue<JOB, true>).
int plan_reads(dyn_batch* b, LaunchPlan& L) {
  dyn_aligner* a = b->a;
  const int32_t* km = b->kmers();
  L.strict_rows.assign(b->n, 0);
  for (uint64_t i = 0; i < b->n; ++i) {
    const HostRead& r = b->reads[i];
    if (r.status != DYN_READ_OK) continue;
    if (a->ntk) continue;  // no read reaches the device; its status is set by init_read_state
    // the banded-lattice kernel (band_reads.hip): the reference's own arithmetic in every cell, no pages. A wide read takes it
    // inside the reference's band, and every read of a guided batch (dyn_batch_set_guide), whatever its N, inside its guide's
    // window (such a batch then has no read for the read queue)
    if (r.wide || b->guided) {
      L.wide.push_back((uint32_t)i);
      continue;
    }
    if (L.calc && a->strict_mode == 2) L.strict_rows[i] = dynplan::STRICT_ALL;
    else if (L.calc && a->strict_mode == 1) L.strict_rows[i] = tie_rows(a->model, km + r.flat_off, r.kc, r.S);
    L.n_strict += L.strict_rows[i] != 0;
    L.order.push_back((uint32_t)i);
  }
  dynplan::cost_order(L.order, [&](uint32_t i) { return b->reads[i].S; }, L.strict_rows.data());
  // the result buffers the job's kernels write whatever its reads are
  if (L.calc) {
    HIP_TRY(a, b->d_segrow.ensure(std::max<uint64_t>(4, b->capacity * 4)));
    HIP_TRY(a, b->d_medhi.ensure(std::max<uint64_t>(8, b->capacity * 8)));
    HIP_TRY(a, b->d_medlo.ensure(std::max<uint64_t>(8, b->capacity * 8)));
  }
  if (L.job == DynJob::Train) {
    HIP_TRY(a, b->d_colw.ensure(std::max<uint64_t>(8, b->total_cols * 8)));
    HIP_TRY(a, b->d_cols1.ensure(std::max<uint64_t>(8, b->total_cols * 8)));
    HIP_TRY(a, b->d_cols2.ensure(std::max<uint64_t>(8, b->total_cols * 8)));
    HIP_TRY(a, b->d_trans.ensure(std::max<uint64_t>(16, b->n * 16)));
    // (the DEVICE-resident pooled statistics -- a radix sort and a segmented sum behind every training launch, 2.4 % of it --
    //  have one reader, dyn_batch_device_pooled for the multi-GPU all-reduce: they are computed when it asks, round 5)
    b->pooled_on_device = false;
  }
  return DYN_OK;
}

// HBM budget for the page pool, page geometry, posterior layout, the initial per-read state (with the reads whose lattice alone
// exceeds the budget) and the pool itself
int size_pool(dyn_batch* b, LaunchPlan& L) {
  dyn_aligner* a = b->a;
  std::vector<uint32_t>& order = L.order;
  L.budget = mem_budget_left(a);
  if (L.lattice) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(a, hipMemGetInfo(&free_b, &total_b));
    // the handle's own pool and the pools destroyed handles have parked on this device are not "free", but they are
    // this launch's to use: without the parked share the budget of a second handle depended on the process's history
    const uint64_t pool = a->ws.bytes + a->lpe.bytes + a->bits.bytes + parked_bytes(a->device);
    const uint64_t avail = (uint64_t)((double)(free_b + pool) * 0.90);
    if (L.budget == 0 || L.budget > avail) L.budget = avail;
  }

  // rows per page: the longest read must fit the waves' PT_MAX-entry page tables
  for (uint32_t i : order) L.max_T = std::max<uint32_t>(L.max_T, (uint32_t)(b->reads[i].S + 1));
  L.log_r = dyneng::min_page_log_rows();
  while (((uint64_t)L.max_T + 1 + ((1ull << L.log_r) - 1)) >> L.log_r > (uint64_t)dynk::PT_MAX) ++L.log_r;
  L.page_rows = 1ull << L.log_r;
  L.n_slots = std::min<size_t>(order.size(), (size_t)a->n_cus * dynk::WAVES_PER_CU);
  auto pages_wanted = [&]() {
    std::vector<uint32_t> pg(order.size());
    for (size_t k = 0; k < order.size(); ++k) pg[k] = L.pages(b, order[k]);
    return dynplan::pages_wanted(pg, L.n_slots);
  };
  uint64_t wanted = pages_wanted();

  L.lpe_separate = L.calc && dynplan::choose_lpe_layout(L.budget, wanted, L.page_rows);
  const uint64_t row_bytes = L.calc ? (L.lpe_separate ? dynplan::row_sep : dynplan::row_inp) : (uint64_t)dynk::P * 8;
  L.page_bytes = L.page_rows * row_bytes;
  L.qjob = L.job == DynJob::Train ? (a->train_zcheck ? dynk::JOB_TRAIN_ZCHECK : dynk::JOB_TRAIN)
           : !L.calc            ? dynk::JOB_Z
           : L.lpe_separate     ? dynk::JOB_ALIGN
                                : dynk::JOB_ALIGN_INPLACE;

  // A read whose lattice alone exceeds the budget fails on its own (the reference would die of std::bad_alloc for that read
  // only, segment.py:172-176), it does not take the batch with it.
  L.st = init_read_state(b, a->ntk);
  if (L.lattice) {
    size_t wr = 0;
    for (uint32_t i : order) {
      if ((uint64_t)L.pages(b, i) * L.page_bytes > L.budget) L.st[i].status = DYN_READ_TOO_LARGE;
      else order[wr++] = i;
    }
    if (wr != order.size()) {
      order.resize(wr);
      wanted = pages_wanted();
    }
  }
  if (b->n) HIP_TRY(a, hipMemcpyAsync(b->d_state.p, L.st, b->n * sizeof(ReadState), hipMemcpyHostToDevice, a->stream));
  L.n_ok = order.size();

  // the pool: grow-only, shared by every batch of the handle (stream order serialises them)
  L.pool.log_rows = L.log_r;
  if (L.lattice && L.n_ok) {
    const bool calc = L.calc, lpe_separate = L.lpe_separate;
    const uint64_t cap_pages = L.budget / L.page_bytes;
    const uint64_t target = std::min<uint64_t>(wanted, cap_pages);
    const uint64_t ws_pp = L.page_rows * dynk::P * 8, lpe_pp = L.page_rows * dynk::P * 4, bits_pp = L.page_rows * dynk::ROW_WORDS * 8;
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
    n_pages = std::min<uint64_t>(n_pages, 0xfffffff0ull >> L.log_r);  // pool rows are 32-bit
    if (a->free_list.bytes < n_pages * 4) {
      HIP_TRY(a, hipStreamSynchronize(a->stream));
      HIP_TRY(a, a->free_list.ensure(n_pages * 4, 1.0));
    }
    L.pool.ws = a->ws.as<double>();
    L.pool.lpe = (calc && lpe_separate) ? a->lpe.as<float>() : nullptr;
    L.pool.bits = calc ? a->bits.as<uint64_t>() : nullptr;
    L.pool.free_list = a->free_list.as<uint32_t>();
    L.pool.n_pages = (uint32_t)n_pages;
  }
  HIP_TRY(a, a->ctl.ensure(dynk::QUEUE_CTL_WORDS * 4, 1.0));
  L.pool.ctl = a->ctl.as<uint32_t>();
  return DYN_OK;
}

// Page-starved launches: the queue order is planned (plan_queue above); `rows` is each read's duration. The planner
// works on a queue in LENGTH order (pages descending). A launch with strict reads is in cost order: when its first
// round does not fit the pool it goes back to length order first -- a strict read costs 1.2x a plain one of its length,
// which matters far less than idle slots in a starved launch (config 3 holds ~50 tie reads in 4 096; round 4's first
// builds skipped the planner for such launches).
void plan_starved_queue(const dyn_batch* b, LaunchPlan& L) {
  std::vector<uint32_t>& order = L.order;
  if (!L.lattice || order.size() <= L.n_slots || std::getenv("DYN_NO_BRIDGE")) return;
  if (L.n_strict) {
    uint64_t first_round = 0;
    for (size_t k = 0; k < L.n_slots; ++k) first_round += L.pages(b, order[k]);
    if (first_round <= L.pool.n_pages) return;
    dynplan::length_order(order, [&](uint32_t i) { return b->reads[i].S; });
  }
  std::vector<uint32_t> need(order.size());
  std::vector<uint64_t> rows(order.size());
  for (size_t k = 0; k < order.size(); ++k) {
    need[k] = L.pages(b, order[k]);
    rows[k] = L.cost(b, order[k]);
  }
  plan_queue(order, need, rows, L.n_slots, L.pool.n_pages);
  // (Dealing the first round's strict reads out across the CUs instead of four to a CU was measured: 50.6 vs 50.9 ms on
  //  cfg2 with 26 % tie reads -- the certified sweeps do not get in each other's way inside a CU. Not kept.)
}

// read descriptors in processing order, pages of the first round reserved here; the descriptors of the banded-lattice kernel's
// reads FOLLOW the queue's (the read queue sees the first n_ok, the per-segment kernels all); the upload
int build_descs(dyn_batch* b, LaunchPlan& L) {
  dyn_aligner* a = b->a;
  const uint64_t half_band = a->model.half_band;
  HIP_TRY(a, b->h_descs.ensure(std::max<size_t>(sizeof(ReadDesc), (L.n_ok + L.wide.size()) * sizeof(ReadDesc))));
  ReadDesc* descs = b->h_descs.as<ReadDesc>();
  bool reserving = true;
  for (size_t k = 0; k < L.order.size(); ++k) {
    const uint32_t i = L.order[k];
    const HostRead& r = b->reads[i];
    ReadDesc d = dynplan::make_desc<ReadDesc>(i, r.S, r.kc, half_band, r.sig_off, r.flat_off, r.seg_off, L.rows_total, L.strict_rows[i]);
    d.n_pages = L.lattice ? L.pages(b, i) : 0;
    if (reserving && k < L.n_slots && (!L.lattice || (uint64_t)L.used_pages + d.n_pages <= L.pool.n_pages)) {
      d.first_page = L.lattice ? L.used_pages : 0;
      L.used_pages += d.n_pages;
      L.n_static = (uint32_t)(k + 1);
    } else {
      reserving = false;  // later reads get their pages on the device
    }
    L.rows_total += d.T;
    L.max_N = std::max(L.max_N, d.N);
    descs[k] = d;
    L.tm.cells += (uint64_t)d.T * std::min<uint64_t>(2ull * d.bw + 1, d.N);
    L.tm.samples += r.S;
  }
  // The banded-lattice kernel's reads: one lattice arena per workgroup, sized for the largest of them (none for Z only).
  // The arenas are the batch's own -- except a self-guided TICKET's (dyn_aligner_set_auto_guide), which uses the handle's: a
  // stream keeps many tickets in flight, each would hold workgroups x its largest lattice until the caller lets go of it (eight
  // tickets of 1 024 reads of 20 k samples at half width 64: 67 GB each), and only the ticket the compute stream is working on
  // needs them. Stream order hands the handle's arenas from one ticket to the next.
  std::vector<uint32_t>& wide = L.wide;
  L.arena_buf = (b->async && b->guided) ? &a->band_arena : &b->d_arena;
  if (!wide.empty()) {
    uint64_t room = 0;
    if (int rc = arena_room(a, *L.arena_buf, b->guided, &room)) return rc;
    size_t wr = 0;
    for (uint32_t i : wide) {
      const HostRead& r = b->reads[i];
      const uint64_t need = dynk::band_arena_bytes(r.S + 1, b->guided ? b->guide_hw : std::min<uint64_t>(a->model.half_band, (r.kc + 1) / 2), L.band_job);
      if (need > room) L.st[i].status = DYN_READ_TOO_LARGE;
      else {
        L.wide_arena = std::max(L.wide_arena, need);
        wide[wr++] = i;
      }
    }
    if (wr != wide.size()) {
      wide.resize(wr);
      if (b->n) HIP_TRY(a, hipMemcpyAsync(b->d_state.p, L.st, b->n * sizeof(ReadState), hipMemcpyHostToDevice, a->stream));
    }
    if (!wide.empty())
      L.wide_groups = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)wide.size(), (uint64_t)a->n_cus * (uint64_t)dynk::band_groups_per_cu(b->guided, (int)b->guide_hw, L.band_job),
                                                                     L.wide_arena ? room / L.wide_arena : ~0ull}));
  }
  b->arena_bytes = 0;
  L.n_all = L.n_ok + L.wide.size();
  for (size_t k = 0; k < L.wide.size(); ++k) {
    const uint32_t i = L.wide[k];
    const HostRead& r = b->reads[i];
    const ReadDesc d = dynplan::make_desc<ReadDesc>(i, r.S, r.kc, half_band, r.sig_off, r.flat_off, r.seg_off, L.rows_total, 0);
    L.rows_total += d.T;
    L.max_N = std::max(L.max_N, d.N);
    descs[L.n_ok + k] = d;
    L.tm.cells += (uint64_t)d.T * (b->guided ? 2ull * b->guide_hw + 1 : std::min<uint64_t>(2ull * d.bw + 1, d.N));
    L.tm.samples += r.S;
  }
  if (L.calc) {
    HIP_TRY(a, b->d_pp.ensure(std::max<uint64_t>(8, L.rows_total * 8)));
    HIP_TRY(a, b->d_pathn.ensure(std::max<uint64_t>(4, L.rows_total * 4)));
  }
  HIP_TRY(a, b->d_descs.ensure(std::max<size_t>(sizeof(ReadDesc), L.n_all * sizeof(ReadDesc))));
  if (L.n_all) HIP_TRY(a, hipMemcpyAsync(b->d_descs.p, descs, L.n_all * sizeof(ReadDesc), hipMemcpyHostToDevice, a->stream));
  return DYN_OK;
}

// ---- the guide rescue: what its stage needs is sized HERE, before anyone knows which reads will be flagged ----
// One lattice arena per workgroup of the refining launch, sized for T_fit: the longest ok read for which at least one arena fits
// what the page pool (allocated above) has left, within the handle's budget. A flagged read above T_fit gets code 2 on the
// device. A ticket's arenas are the handle's, handed from ticket to ticket in stream order (as a self-guided ticket's are, and
// for its reason); a synchronous batch's are the batch's own, shared with its wide reads' launch, which has ended by then.
int size_rescue(dyn_batch* b, LaunchPlan& L) {
  dyn_aligner* a = b->a;
  L.resc_arena_buf = b->async ? &a->band_arena : &b->d_arena;
  if (!L.rescue || !L.n_all) return DYN_OK;
  const ReadDesc* descs = b->h_descs.as<ReadDesc>();
  uint64_t room = 0;
  if (int rc = arena_room(a, *L.resc_arena_buf, true, &room)) return rc;
  for (size_t k = 0; k < L.n_all; ++k)
    if (descs[k].T > L.resc_T_fit && dynk::band_arena_bytes(descs[k].T, b->want.rescue_hw, 1) <= room) L.resc_T_fit = descs[k].T;
  if (L.resc_T_fit) {
    L.resc_arena = dynk::band_arena_bytes(L.resc_T_fit, b->want.rescue_hw, 1);
    L.resc_groups = (int)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)L.n_all, (uint64_t)a->n_cus * (uint64_t)dynk::band_groups_per_cu(true, (int)b->want.rescue_hw, 1),
                                                                   room / L.resc_arena}));
    L.resc_want = 256 + (uint64_t)L.resc_groups * L.resc_arena;
  }
  return DYN_OK;
}

// per-read rescaling (dyn_aligner_set_rescale): align(calc = 1) runs 1 + iters passes of the launches, in stream order
int prepare_rescale(dyn_batch* b, LaunchPlan& L) {
  dyn_aligner* a = b->a;
  const int iters = L.n_pass - 1;
  HIP_TRY(a, b->h_stats.ensure((size_t)L.n_pass * dynk::QUEUE_CTL_WORDS * 4));
  std::memset(b->h_stats.p, 0, (size_t)L.n_pass * dynk::QUEUE_CTL_WORDS * 4);
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
  if (iters) {
    const uint64_t head = (b->n * sizeof(dynk::RescaleState) + 255) / 256 * 256;
    HIP_TRY(a, b->d_rs.ensure(std::max<uint64_t>(256, head + b->capacity * 8)));
    L.rs = b->d_rs.as<dynk::RescaleState>();
    L.rs_y = reinterpret_cast<double*>(b->d_rs.as<char>() + head);
    dynk::launch_rescale_init(L.rs, b->n, a->stream);
  }
  b->n_passes = L.n_pass;
  return DYN_OK;
}

// the batch's events, the read queue's arguments and the four outputs the lattice phases write
int prepare_lattice_outputs(dyn_batch* b, const LaunchPlan& L, dynk::QueueArgs& q) {
  dyn_aligner* a = b->a;
  const PoreModel& m = a->model;
  const bool calc = L.calc;
  while (b->events.size() < 3) {
    hipEvent_t e = nullptr;
    HIP_TRY(a, hipEventCreate(&e));
    b->events.push_back(e);  // owned by the batch from here on: destroyed with it whatever happens next
  }
  q.descs = b->d_descs.as<ReadDesc>();
  q.n_reads = (int)L.n_ok;
  q.n_static = (int)L.n_static;
  q.sig = b->d_sig.as<double>();
  q.par = b->d_par.as<Emis>();
  q.pool = L.pool;
  q.st = b->d_state.as<ReadState>();
  q.tb = dynk::TraceBuffers{b->d_pp.as<double>(), b->d_pathn.as<uint32_t>(), b->d_segrow.as<uint32_t>(), b->d_medhi.as<double>(), b->d_medlo.as<double>()};
  // (train jobs only: in an align job the posterior samples take their place, below)
  if (L.job == DynJob::Train) q.tr = dynk::TrainBuffers{b->d_colw.as<double>(), b->d_cols1.as<double>(), b->d_cols2.as<double>(), b->d_trans.as<double>()};
  q.m1 = m.log_m1;
  q.e2 = m.log_e2;
  q.sp_tab = a->d_sptab.as<dynmath::SoftplusNode>();
  q.z_fail_status = L.z_fail;
  q.lpe_floor = a->lpe_floor;
  q.lpe_dense = a->lpe_dense ? 1 : 0;
  // The four outputs of the lattice phases, each zeroed here (rows of reads that fail keep the zeros) and written by the read queue /
  // the banded-lattice kernel of the LAST pass behind every read (run_pass):
  //   per-border posterior confidence  [border_probability | border_window_probability] x capacity
  //   credible intervals               [mean | sd] f64 and [lo | hi] u32 x capacity in one buffer
  //   soft levels                      [weight | sum | sumsq] f64 x capacity in one buffer
  //   posterior path samples           [count][capacity] segment starts, then the per-read count of dead samples. (The callers
  //                                    refuse the switches that would make this more than one pass.)
  for (Output k : {OUT_BORDERS, OUT_INTERVALS, OUT_SOFT, OUT_SAMPLES})
    if (int rc = output_prepare(b, k, calc ? output_wanted(b->want, k) : 0, a->stream)) return rc;
  if (b->out[OUT_SAMPLES].ready) {
    q.sample.start = b->out[OUT_SAMPLES].d.as<uint32_t>();  // (the dead counts follow the planes)
    q.sample.capacity = b->capacity;
    q.sample.seed = b->want.sample_seed;
    q.sample.count = b->want.posterior_samples;
    q.lpe_dense = 1;  // a sampled path may visit any cell of the band (the kernel variant that carries the phase stores densely anyway)
  }
  if (!b->ev_done) HIP_TRY(a, hipEventCreateWithFlags(&b->ev_done, hipEventDisableTiming));
  return DYN_OK;
}

// guide refinement (dyn_batch_set_guide_refine) of a synchronous batch: behind every alignment a step that makes the called path
// the next guide of the reads whose guide it does not reproduce, and the list of those reads the next alignment's queue. Every
// round is enqueued; a round whose list is empty ends at its first queue read. What follows the traceback
// (launch_segments and the riders) runs once, behind the last round. `ba`'s first alignment has been launched by the caller.
int run_refine_rounds(dyn_batch* b, const LaunchPlan& L, const dynk::QueueArgs& q, dynk::BandArgs ba) {
  dyn_aligner* a = b->a;
  const uint64_t nb = b->n, nw = L.wide.size();
  HIP_TRY(a, b->d_gref.ensure((2 * nb + 64 + 2 * nw) * 4));
  uint32_t* g = b->d_gref.as<uint32_t>();
  HIP_TRY(a, hipMemsetAsync(g, 0, 2 * nb * 4, a->stream));
  uint32_t* cnt[2] = {g + 2 * nb, g + 2 * nb + 32};
  uint32_t* act[2] = {g + 2 * nb + 64, g + 2 * nb + 64 + nw};
  // descs, n_reads, st | pathn, segrow | guide | rounds, converged; the lists and `last` per round below
  dynk::GuideRefine gr{ba.descs, ba.n_reads, q.st, q.tb.pathn, q.tb.segrow, b->d_guide.as<int32_t>(), g, g + nb};
  for (uint32_t r = 0; r < L.refine_rounds; ++r) {
    if (r > 0) {
      ba.active = act[(r - 1) & 1];
      ba.n_active = cnt[(r - 1) & 1];
      HIP_TRY(a, dynk::launch_band_reads(L.band_job, ba, L.wide_groups, a->stream));
    }
    gr.active_in = ba.active;
    gr.n_in = ba.n_active;
    gr.active_out = act[r & 1];
    gr.n_out = cnt[r & 1];
    gr.last = r + 1 == L.refine_rounds ? 1 : 0;
    HIP_TRY(a, dynk::launch_guide_refine(gr, a->stream));
  }
  b->gref_ready = true;
  return DYN_OK;
}

// the banded-lattice kernel's reads: a queue of its own behind the read queue on the compute stream (its results feed the same
// per-segment kernels / the same host finalisation)
int launch_wide(dyn_batch* b, const LaunchPlan& L, const dynk::QueueArgs& q, int pass) {
  dyn_aligner* a = b->a;
  DevBuf& arena_buf = *L.arena_buf;
  if (pass == 0) {
    // (a synchronous batch under the guide rescue: the rescue stage works in the same buffer, which must not grow again)
    const uint64_t want = std::max<uint64_t>(256 + (uint64_t)L.wide_groups * L.wide_arena, L.arena_buf == L.resc_arena_buf ? L.resc_want : 0);
    if (int rc = grow_arena(a, arena_buf, want)) return rc;
    b->arena_bytes = (uint64_t)L.wide_groups * L.wide_arena;
  }
  dynk::BandArgs ba = band_args_common(b, q, L.z_fail, arena_buf, L.wide_arena);
  ba.descs = q.descs + L.n_ok;
  ba.n_reads = (int)L.wide.size();
  ba.bw = (int)b->guide_hw;
  ba.guide = b->guided ? b->d_guide.as<int32_t>() : nullptr;  // null: the diagonal window
  ba.tr = q.tr;  // (an align job: the posterior samples, the credible intervals or the soft levels, which share the place)
  ba.border_window = q.border_window;  // (guided batches refuse the rider: dynamont_mi.cpp)
  ba.border_p = q.border_p;
  ba.border_window_p = q.border_window_p;
  // A TICKET that refines (dyn_aligner_set_auto_guide): ONE launch in which the workgroup that holds a read aligns it until
  // its guide reproduces itself (BandArgs::refine_rounds) -- a launch per round lasts as long as its longest read however
  // few reads are still open, which a stream of tickets cannot afford. The synchronous batch keeps the round scheme
  // (run_refine_rounds): it is what the refining launch is checked against, bit for bit.
  const bool refine_in_launch = L.refine_rounds > 1 && b->async;
  if (refine_in_launch) {
    HIP_TRY(a, b->d_gref.ensure(std::max<uint64_t>(8, 2 * b->n * 4)));
    HIP_TRY(a, hipMemsetAsync(b->d_gref.p, 0, 2 * b->n * 4, a->stream));
    ba.refine_rounds = (int)L.refine_rounds;
    ba.rounds = b->d_gref.as<uint32_t>();
    ba.converged = b->d_gref.as<uint32_t>() + b->n;
    b->gref_ready = true;
  }
  HIP_TRY(a, dynk::launch_band_reads(L.band_job, ba, L.wide_groups, a->stream));
  if (L.refine_rounds > 1 && !refine_in_launch) return run_refine_rounds(b, L, q, ba);
  return DYN_OK;
}

// One pass: it resets what a launch resets -- per-read state, queue head and page pool (k_pool_init), the banded-lattice kernel's
// head (launch_band_reads) -- then the read queue, the statistics copy, the banded-lattice kernel and, between two passes, the fit.
int run_pass(dyn_batch* b, const LaunchPlan& L, dynk::QueueArgs& q, int pass) {
  dyn_aligner* a = b->a;
  hipEvent_t* ev = b->events.data();
  const bool last = pass + 1 == L.n_pass;
  if (pass > 0 && b->n) HIP_TRY(a, hipMemcpyAsync(b->d_state.p, L.st, b->n * sizeof(ReadState), hipMemcpyHostToDevice, a->stream));
  dynk::launch_pool_init(L.pool, L.used_pages, (int)L.n_static, a->stream);
  // the lattice phases of the last pass: each reads whole windows or columns of LPE (the kernel variant that carries it stores
  // densely anyway). The callers refuse the interval beside the border confidence or the samples, the soft levels beside all three.
  if (last && b->out[OUT_BORDERS].ready) {
    q.border_window = b->want.border_confidence;
    q.border_p = b->out[OUT_BORDERS].d.as<double>();
    q.border_window_p = q.border_p + b->capacity;
  }
  if (last && b->out[OUT_INTERVALS].ready) q.interval = dynk::IntervalOut{b->out[OUT_INTERVALS].d.as<double>(), b->capacity, (1.0 - b->want.border_interval) / 2, 0};
  if (last && b->out[OUT_SOFT].ready) q.soft = dynk::SoftOut{b->out[OUT_SOFT].d.as<double>(), b->capacity, 0, dynk::SOFT_TAG};
  if (last && (b->out[OUT_BORDERS].ready || b->out[OUT_INTERVALS].ready || b->out[OUT_SOFT].ready)) q.lpe_dense = 1;
  if (pass == 0) HIP_TRY(a, hipEventRecord(ev[0], a->stream));
  HIP_TRY(a, dynk::launch_read_queue(L.qjob, L.n_strict != 0, q, a->n_cus, a->stream));
  if (last) HIP_TRY(a, hipEventRecord(ev[1], a->stream));
  // the statistics leave the control words before the next pass's or batch's k_pool_init resets them (same stream)
  HIP_TRY(a, hipMemcpyAsync(b->h_stats.as<uint32_t>() + (size_t)pass * dynk::QUEUE_CTL_WORDS, L.pool.ctl, dynk::QUEUE_CTL_WORDS * 4,
                            hipMemcpyDeviceToHost, a->stream));
  // (Running the per-segment kernels on a stream of their own, beside the next batch's read queue, was measured:
  //  the 0.35 ms gap it closes comes back as a 0.4 ms slower start of that read queue -- same-box A/B, no gain.)
  if (!L.wide.empty())
    if (int rc = launch_wide(b, L, q, pass)) return rc;
  // between two passes: the fit of every read and its signal recomputed from x0. (The per-segment kernels run once, after
  // the last pass: the fit reads the borders the traceback wrote, segrow, and nothing of k_median / k_final.)
  if (!last)
    dynk::launch_rescale_pass(q.descs, (int)L.n_all, L.max_T, q.st, q.tb, b->d_sig0.as<double>(), b->d_sig.as<double>(), q.par, L.rs_y, L.rs, a->stream);
  return DYN_OK;
}

// ---- the guide rescue stage: behind the read queue and the diagonal banded-lattice launch, in front of the riders ----
// (guide_rescue_kernels.hpp lists the launches). The host waits for none of them: a ticket's front thread enqueues the lot.
int run_rescue(dyn_batch* b, const LaunchPlan& L, const dynk::QueueArgs& q) {
  dyn_aligner* a = b->a;
  const int nr_all = (int)L.n_all;
  const uint64_t nb = b->n;
  const uint64_t off_code = 2 * nb * 4, off_len = (off_code + nb + 255) / 256 * 256, off_list = off_len + 256;
  const uint64_t off_bm = off_list + (uint64_t)L.n_all * 4;
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
  dynk::launch_band_margin(q.descs, nr_all, L.max_N, q.st, q.tb, dm, a->stream);
  // descs, n_reads, st | low, high | min_margin, max_T | code, list, n_list
  const dynk::RescueSelect sel{q.descs, nr_all, q.st, dm.low, dm.high, b->want.rescue_margin, L.resc_T_fit, g_code, g_list, g_len};
  HIP_TRY(a, dynk::launch_rescue_select(sel, a->stream));
  if (!L.resc_T_fit || !nr_all) return DYN_OK;
  // the guide (zero-filled, one int32 per sample of the batch) and the pre-pass's queue head behind it
  const uint64_t total = b->reads[b->n - 1].sig_off + b->reads[b->n - 1].S;
  const uint64_t head_off = (total * 4 + 255) / 256 * 256;
  HIP_TRY(a, b->d_guide.ensure(head_off + 256));
  if (total) HIP_TRY(a, hipMemsetAsync(b->d_guide.p, 0, total * 4, a->stream));
  // descs, n_reads, bw | sig, par | guide, head | m1, e2 | active, n_active
  const dynk::AutoGuideArgs ag{q.descs, nr_all, (int)b->want.rescue_hw, q.sig, q.par, b->d_guide.as<int32_t>(),
                               reinterpret_cast<uint32_t*>(b->d_guide.as<char>() + head_off), a->model.log_m1, a->model.log_e2, g_list, g_len};
  const int ag_groups = (int)std::min<uint64_t>(L.n_all, (uint64_t)a->n_cus * (uint64_t)dynk::auto_guide_groups_per_cu((int)b->want.rescue_hw));
  HIP_TRY(a, dynk::launch_auto_guide(ag, ag_groups, a->stream));
  // the rescue alignment writes a state, path rows and segment rows of its OWN (the read's offsets, other buffers): the
  // plain answer stays whole until launch_rescue_merge has seen how the rescue ended
  HIP_TRY(a, b->d_resc_st.ensure(std::max<uint64_t>(sizeof(ReadState), nb * sizeof(ReadState))));
  HIP_TRY(a, b->d_resc_pp.ensure(std::max<uint64_t>(8, L.rows_total * 8)));
  HIP_TRY(a, b->d_resc_pathn.ensure(std::max<uint64_t>(4, L.rows_total * 4)));
  HIP_TRY(a, b->d_resc_segrow.ensure(std::max<uint64_t>(4, b->capacity * 4)));
  if (int rc = grow_arena(a, *L.resc_arena_buf, L.resc_want)) return rc;
  b->arena_bytes = std::max<uint64_t>(b->arena_bytes, L.resc_want - 256);
  dynk::BandArgs ra = band_args_common(b, q, L.z_fail, *L.resc_arena_buf, L.resc_arena);
  ra.n_reads = nr_all;
  ra.bw = (int)b->want.rescue_hw;
  ra.guide = b->d_guide.as<int32_t>();
  ra.st = b->d_resc_st.as<ReadState>();
  ra.tb = dynk::TraceBuffers{b->d_resc_pp.as<double>(), b->d_resc_pathn.as<uint32_t>(), b->d_resc_segrow.as<uint32_t>(), nullptr, nullptr};
  ra.active = g_list;
  ra.n_active = g_len;
  ra.refine_rounds = (int)b->want.rescue_rounds;
  ra.rounds = g_rounds;
  ra.converged = g_conv;
  HIP_TRY(a, dynk::launch_band_reads(1, ra, L.resc_groups, a->stream));
  // descs, n_reads | list, n_list | the rescue's st, pp, pathn, segrow | the job's own | code, rounds, converged | single
  const dynk::RescueMerge mg{q.descs, nr_all, g_list, g_len, ra.st, ra.tb.pp, ra.tb.pathn, ra.tb.segrow, q.st, q.tb.pp, q.tb.pathn, q.tb.segrow,
                             g_code, g_rounds, g_conv, b->want.rescue_rounds <= 1 ? 1 : 0};
  HIP_TRY(a, dynk::launch_rescue_merge(mg, a->stream));
  // a rescued read reports its margins against the window it was aligned in, every other read against the diagonal (above)
  if (b->bm_ready)
    dynk::launch_guided_band_margin(q.descs, nr_all, b->max_T, q.st, q.tb, b->d_guide.as<int32_t>(), (int)b->want.rescue_hw, dm, a->stream, g_code);
  return DYN_OK;
}

// the events behind the job, and what the batch remembers of it
int finish(dyn_batch* b, LaunchPlan& L) {
  dyn_aligner* a = b->a;
  if (L.job == DynJob::Train) {
    b->pool_nr = (int)L.n_all;
    b->pool_max_N = L.max_N;
  }
  HIP_TRY(a, hipEventRecord(b->events[2], a->stream));
  HIP_TRY(a, hipEventRecord(b->ev_done, a->stream));
  HIP_TRY(a, hipGetLastError());
  dyn_timing& tm = L.tm;
  const uint32_t launches = (L.n_ok || !L.wide.empty()) ? 1 : 0;
  tm.launch_share = 1.0;
  tm.launches = launches;
  tm.lp_inplace = (L.calc && !L.lpe_separate) ? 1 : 0;
  tm.pool_pages = L.pool.n_pages;
  tm.page_rows = (uint32_t)L.page_rows;
  tm.n_static = L.n_static;
  tm.n_waves = (uint32_t)std::min<size_t>((L.order.size() + dynk::WAVES_PER_CU - 1) / dynk::WAVES_PER_CU * dynk::WAVES_PER_CU,
                                         (size_t)a->n_cus * dynk::WAVES_PER_CU);
  record_job(b, tm, L.job, L.calc, L.n_all, L.n_strict, L.strict_rows, launches);
  return DYN_OK;
}

}  // namespace

int enqueue_job(dyn_batch* b, DynJob job) {
  dyn_aligner* a = b->a;
  LaunchPlan L;
  L.job = job;
  L.lattice = job != DynJob::AlignZ;
  L.calc = job == DynJob::AlignFull;
  L.z_fail = job == DynJob::Train ? DYN_READ_TRAIN_Z_MISMATCH : DYN_READ_Z_MISMATCH;
  L.band_job = job == DynJob::Train ? 2 : L.calc ? 1 : 0;  // launch_band_reads' job
  L.refine_rounds = (b->guided && L.calc) ? b->guide_refine : 1;  // dyn_batch_set_guide_refine
  L.n_pass = 1 + (L.calc ? b->want.rescale_iters : 0);            // dyn_aligner_set_rescale
  // the guide rescue (dyn_aligner_set_guide_rescue): sampled per job by the caller; it concerns the unguided align job with
  // probabilities alone (the callers refuse the combinations with rescale / border confidence / a guide)
  L.rescue = L.calc && b->want.rescue_hw > 0 && !b->guided && !a->ntk && b->want.rescale_iters == 0 && b->want.border_confidence == 0;
  b->gref_ready = b->gr_ready = false;

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

  if (int rc = plan_reads(b, L)) return rc;
  if (int rc = size_pool(b, L)) return rc;
  plan_starved_queue(b, L);
  if (int rc = build_descs(b, L)) return rc;
  if (int rc = size_rescue(b, L)) return rc;
  if (int rc = prepare_rescale(b, L)) return rc;
  dynk::QueueArgs q{};
  if (int rc = prepare_lattice_outputs(b, L, q)) return rc;
  for (int pass = 0; pass < L.n_pass; ++pass)
    if (int rc = run_pass(b, L, q, pass)) return rc;
  if (int rc = band_margin_prepare(b, L.calc)) return rc;
  if (L.rescue) {
    if (int rc = run_rescue(b, L, q)) return rc;
    b->gr_ready = true;
  }
  for (Output k : {OUT_LEVELS, OUT_SCORES, OUT_SITE_CALLS})
    if (int rc = output_prepare(b, k, L.calc ? output_wanted(b->want, k) : 0, a->stream)) return rc;
  // (under the guide rescue the margins were taken by its stage, in front of the selection: such a job is never a merged launch;
  //  a guided batch's are taken against its own window)
  if (L.calc)
    enqueue_riders(b, q.descs, (int)L.n_all, L.rows_total, L.max_N, q.st, q.tb, a->stream,
                   L.rescue ? Margins::Taken : b->guided ? Margins::Guided : Margins::Diagonal);
  return finish(b, L);
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
