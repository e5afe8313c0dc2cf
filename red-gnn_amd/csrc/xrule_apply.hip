// Application of weighted extrapolation rules to queries (include/redgnn.h: rg_xrule_apply): for every query (s, r, ?, day t) and
// entity y, which of the rules with head r connect s to y through rows that each step admits for day t, folded in rule order into
// (best weight, its rule, product of the misses, number of rules that fired).
//
// Two designs put together.  From trule_apply.hip the per-rule slabs (rule_slabs.h): a rule's columns are only the queries of its head
// relation, its two bitmaps are slabs of n_ent * W_i words at word slab[i] of the two regions of the scratch, and the seed and the
// aggregate - the fold - are taken from the header.  From xrule_ground.hip the window-tested day walk: a step (r, [lo, hi)) admits
//   the data row j = (u, r, v) at day t      iff  win_lo[t] <= j < win_hi[t]  and  lo <= t - row_day[j] < hi
//   the self-loop (u, n_rel_true, u) at t    iff  lo <= min(t, loop_window) < hi
// exactly as that file admits them for an anchor of day t; there is no head pass.
//
// Queries.  The host sorts them stably by (relation, day).  q_ptr int32 [n_rela_rows + 1] has one entry per relation, as rg_rule_apply
// has it, so the slabs, the seed and the aggregate work as they are: relation h owns the sorted positions p0 = q_ptr[h] .. p1 =
// q_ptr[h + 1] and bit c of a rule of head h is the query at position p0 + c.  The days are not an index of q_ptr (n_rela_rows * n_day
// entries for a batch that covers a few days) and the hop does not walk a step's candidate days (xrule_ground tests every later day
// of a row for an open bin).  Instead the host lists the distinct query days of every relation, the "entries":
//   day_ptr int32 [n_rela_rows + 1]   relation h owns the entries day_ptr[h] .. day_ptr[h + 1]
//   day_of  int32 [D]                 the day of every entry, ascending inside a relation
//   day_pos int32 [D + 1]             the first sorted position of every entry; day_pos[D] = batch
// Entry k of relation h owns the columns [day_pos[k] - p0, day_pos[k + 1] - p0): the end of a relation's last entry is the first
// position of the next relation.  Entries are adjacent in columns even where their days are not - the days between hold no query.
//
//   fill       the whole scratch is zeroed by rg::zero_async
//   seed       apply_seed_kernel: bit c of cur_i[q_sub[p0 + c]]
//   hop l      the edges of relation body[i][l] under [lag_lo[i][l], lag_hi[i][l]):
//              data row j of day d   the candidate days are [d + lo, min(d + hi, n_day)); the first entry of h whose day is >= the first
//                                    candidate day is found by binary search, the entries are walked while their day is below the last,
//                                    each entry's day is tested against its window, and every run of consecutive passing entries
//                                    [run, k) moves the one column range [day_pos[run] - p0, day_pos[k] - p0)
//              self-loop             the days that pass are one range [a, b) (xrule_ground's formula): two binary searches, one range
//              with the both-end masks and the integer atomicOr of move_range (rule_bits.h).  Work per edge: O(log D_h + entries in
//              range), not n_day.  Then cur <-> next, and the new next is zeroed before the next hop
//   aggregate  apply_aggregate_kernel, one entry of q_ptr per relation
//
// Lanes.  The rule is blockIdx.y and a group of G lanes owns one edge: every lane of the group walks the edge's entries (the same
// addresses for the group) and the group strides over the words of a run.  A workgroup has one rule and one step, so it picks G
// itself: the power of two >= the words a run can span, min(hi - lo, loop_window + 1) days at W_i / span_h words a day plus one
// (span_h: the days from relation h's first query day to its last), at most the power of two >= W_i, at most 64.  A relation whose
// first edge is a self-loop (the identity relation holds nothing else) takes the row-wide group: its one range is most of the row.
// A range wider than G is walked in strides of G, so every G is correct (-DRG_XRULE_APPLY_ONE_G: the row-wide group for every step,
// the A/B build of tools/build_variant.sh).  The grid is sized from the widest rule there can be.
//
// Determinism.  OR is order-independent and the fold's order is the rule order: every output is the same bit for bit in every run, for
// every grid and every G, and however the rules are cut into consecutive calls.
//
// Bounds.  A relation id outside 0..n_rela_rows-1 (head or step) is tested before any load and reads nothing; lag_lo >= lag_hi makes
// the step empty; an edge end or subject outside 0..n_ent-1, a row index outside 0..n_data, a row_day or day_of value outside
// 0..n_day-1 and a q_row outside 0..batch-1 are skipped; the candidate days are formed in int64 and clamped to 0..n_day before any
// window entry is read; day_ptr entries are clamped to 0..D, day_pos and q_ptr entries to 0..batch and every range to 0..S_i, and a
// range with lo >= hi moves nothing; a slab that does not lie inside 0..n_words is left out.  The binary searches stay inside the
// relation's clamped entries whatever day_of holds (an unsorted day_of makes the rules of that head unspecified, nothing else).  The
// bits of a slab's last word beyond S_i are never set by the seed and a hop only moves bits.  Whatever the arrays hold, nothing
// outside the graph, row_day[0..n_data), win_lo / win_hi[0..n_day), the query arrays, the scratch or the four outputs is touched.
#include "rule_slabs.h"

namespace {

using namespace rgapply;

struct QueryDays {
  const int32_t* ptr;      // [n_rela_rows + 1] entries by relation
  const int32_t* day;      // [D] the day of every entry, ascending inside a relation
  const int32_t* pos;      // [D + 1] the first sorted position of every entry
  int32_t D;
};

struct Windows {
  const int32_t* row_day;  // [n_data]
  const int32_t* lo;       // [n_day]
  const int32_t* hi;       // [n_day]
  int32_t n_data, n_day, loop_window;
};

// the first entry k in [k0, k1) whose day is >= t, k1 if none
__device__ __forceinline__ int32_t first_entry(const int32_t* __restrict__ day_of, int32_t k0, int32_t k1, int32_t t) {
  while (k0 < k1) {
    const int32_t mid = k0 + ((k1 - k0) >> 1);
    if (day_of[mid] < t) k0 = mid + 1; else k1 = mid;
  }
  return k0;
}

// step l of every rule: to_i[v] |= from_i[u] & columns(entries whose day the step admits the edge at) over the edges (u, v, j) of
// relation body[i][l] under the lags [lag_lo[i][l], lag_hi[i][l]).  No barrier: a workgroup whose rule has no query, no such
// relation, an empty lag range, or fewer edges than the grid covers, leaves.
__global__ __launch_bounds__(RT) void xapply_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht,
                                                        const int32_t* __restrict__ rel_tm, Queries q, QueryDays qd, Windows win,
                                                        const int32_t* __restrict__ head, const int32_t* __restrict__ body,
                                                        const int32_t* __restrict__ lo_of, const int32_t* __restrict__ hi_of,
                                                        int32_t n_hops, int32_t l, const int64_t* __restrict__ slab, int32_t n_ent,
                                                        int64_t n_words, const uint32_t* __restrict__ from, uint32_t* __restrict__ to) {
  const int64_t i = blockIdx.y;
  const int32_t r = body[i * n_hops + l];
  if (r < 0 || r >= q.n_rela_rows) return;
  const int64_t lag_lo = lo_of[i * n_hops + l], lag_hi = hi_of[i * n_hops + l];
  if (lag_lo >= lag_hi) return;
  const int32_t h = head[i];
  Slab sl;
  if (!rule_slab(q, h, slab, i, n_ent, n_words, &sl)) return;          // h is in 0..n_rela_rows-1 from here on
  const int32_t W = sl.W, S = sl.S, n_day = win.n_day, n_data = win.n_data;
  const int32_t k0 = min(max(qd.ptr[h], 0), qd.D), k1 = min(max(qd.ptr[h + 1], 0), qd.D);
  if (k0 >= k1) return;
  const int64_t e0 = rel_ptr[r], e1 = rel_ptr[r + 1];
  if (e0 >= e1) return;
  // the lanes of an edge (the file comment): by the widest run of the step, row-wide for the identity relation
  int32_t g_shift = group_shift(W);
#ifndef RG_XRULE_APPLY_ONE_G           // the A/B build (tools/build_variant.sh) keeps the row-wide group for every step
  if (rel_tm[e0] != n_data) {
    const int64_t days = std::min<int64_t>(lag_hi - lag_lo, (int64_t)win.loop_window + 1);
    const int64_t span = std::max<int64_t>((int64_t)qd.day[k1 - 1] - qd.day[k0] + 1, 1);
    g_shift = group_shift(std::min<int64_t>(W, W * days / span + 1));
  }
#endif
  const Lanes ln = hop_lanes(g_shift);
  const auto col_at = [&](int32_t k) { return min(max(clamp_pos(qd.pos[k], q.batch) - sl.p0, 0), S); };      // k in 0..D
  for (int64_t e = e0 + ln.first; e < e1; e += ln.step) {
    const int2 ht = rel_ht[e];
    const int32_t j = rel_tm[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent || (uint32_t)j > (uint32_t)n_data) continue;
    const uint32_t* __restrict__ src = from + sl.base + (int64_t)ht.x * W;
    uint32_t* dst = to + sl.base + (int64_t)ht.y * W;
    if (j == n_data) {                          // a self-loop: the days with lag_lo <= min(t, loop_window) < lag_hi are one range
      if (lag_lo > win.loop_window) continue;
      const int32_t a = (int32_t)std::min<int64_t>(std::max<int64_t>(lag_lo, 0), n_day);
      const int32_t b = lag_hi > win.loop_window ? n_day : (int32_t)std::min<int64_t>(lag_hi, n_day);      // (lag_hi <= 0: a >= b)
      if (a >= b) continue;
      const int32_t ka = first_entry(qd.day, k0, k1, a);
      const int32_t lo = col_at(ka), hi = col_at(first_entry(qd.day, ka, k1, b));
      if (lo < hi) move_range(src, dst, nullptr, lo, hi, ln);
      continue;
    }
    const int32_t d = win.row_day[j];
    if ((uint32_t)d >= (uint32_t)n_day) continue;
    const int32_t t0 = (int32_t)std::min<int64_t>(std::max<int64_t>(d + lag_lo, 0), n_day);
    const int32_t t1 = (int32_t)std::min<int64_t>(std::max<int64_t>(d + lag_hi, 0), n_day);
    if (t0 >= t1) continue;
    int32_t run = -1;                           // the first entry of the current run of passing entries
    int32_t k = first_entry(qd.day, k0, k1, t0);
    for (; k < k1; ++k) {
      const int32_t t = qd.day[k];
      if (t >= t1) break;                       // t1 <= n_day: a day beyond the last ends the walk
      const bool pass = t >= 0 && win.lo[t] <= j && j < win.hi[t];
      if (pass) {
        if (run < 0) run = k;
      } else if (run >= 0) {
        const int32_t lo = col_at(run), hi = col_at(k);
        if (lo < hi) move_range(src, dst, nullptr, lo, hi, ln);
        run = -1;
      }
    }
    if (run >= 0) {
      const int32_t lo = col_at(run), hi = col_at(k);
      if (lo < hi) move_range(src, dst, nullptr, lo, hi, ln);
    }
  }
}

}  // namespace

extern "C" int rg_xrule_apply(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* lag_lo, const int32_t* lag_hi,
                              const float* weight, const float* miss, int32_t n_rules, int32_t n_hops, int32_t rule_base,
                              const int32_t* row_day, int32_t n_data, const int32_t* win_lo, const int32_t* win_hi, int32_t n_day,
                              int32_t loop_window, const int32_t* q_sub, const int32_t* q_row, const int32_t* q_ptr,
                              const int32_t* day_ptr, const int32_t* day_of, const int32_t* day_pos, int32_t n_qdays, int32_t batch,
                              const int64_t* slab, int64_t n_words, void* scratch, int32_t phases, float* best, float* surv,
                              int32_t* best_rule, int32_t* fired, void* stream) {
  RG_CHECK(g, "rg_xrule_apply: NULL graph");
  RG_CHECK(n_data >= 0 && g->n_time != 0 && (int64_t)g->n_time == (int64_t)n_data + 1,
           "rg_xrule_apply: not the extrapolation layout (n_time=%d, n_data=%d: every edge's time field is its data row, n_time = n_data + 1)",
           g->n_time, n_data);
  RG_CHECK(g->rel_ptr && g->rel_ht && g->rel_tm,
           "rg_xrule_apply: the graph has no CSR by relation with edge times (rel_ptr / rel_ht / rel_tm is NULL)");
  if (apply_check("rg_xrule_apply", n_rules, n_hops, batch, phases, rule_base)) return 1;
  RG_CHECK(n_day >= 1, "rg_xrule_apply: n_day=%d", n_day);
  RG_CHECK(loop_window >= 0, "rg_xrule_apply: loop_window=%d", loop_window);
  RG_CHECK(n_qdays >= 0, "rg_xrule_apply: n_qdays=%d", n_qdays);
  if (n_rules == 0 || batch == 0) return 0;
  const Queries q{q_sub, q_row, q_ptr, batch, g->n_rela_rows, 1};
  const QueryDays qd{day_ptr, day_of, day_pos, n_qdays};
  const Windows win{row_day, win_lo, win_hi, n_data, n_day, loop_window};
  const Rules r{head, weight, miss, n_rules, n_hops, rule_base, slab, n_words, best, surv, best_rule, fired};
  const auto hop = [&](int32_t l, dim3 grid, hipStream_t s, const uint32_t* from, uint32_t* to) {
    hipLaunchKernelGGL(xapply_hop_kernel, grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, g->rel_tm, q, qd, win, head, body, lag_lo, lag_hi,
                       n_hops, l, slab, g->n_ent, n_words, from, to);
  };
  return apply_chain("rg_xrule_apply", g, q, r,
                     head && body && lag_lo && lag_hi && weight && miss && (row_day || n_data == 0) && win_lo && win_hi && q_sub &&
                         q_row && q_ptr && day_ptr && (day_of || n_qdays == 0) && day_pos && slab && scratch && best && surv &&
                         best_rule && fired,
                     scratch, phases, stream, hop);
}
