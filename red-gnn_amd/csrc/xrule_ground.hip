// Grounding of extrapolation rules on the one-graph layout of the forecasting model (include/redgnn.h: rg_xrule_ground): for every rule
// (head h, body (r_1, [lo_1, hi_1)) .. (r_L, [lo_L, hi_L))) - a step is a relation and a range of lags in days - and a set of anchors
// (x, t) - an entity and a query day - how many pairs ((x, t), y) the body connects, and how many of those are facts (x, h, y) of day t.
//
// The graph is extrapolation.T_RED_GNN's: the self-loops (relation n_rel_true, time field n_data) and then the data rows, each with its
// own row index j as time field (so g->n_time == n_data + 1).  row_day[j] is the row's day; a query day t sees the rows of its window
// [win_lo[t], win_hi[t]).  The windows keep the reference's quirks (the offset of a day is the index of the LAST row of the day before,
// and 0 after a day without rows), so they are NOT monotone in t and rows with a lag far above the window length occur.  A step
// (r, [lo, hi)) admits
//   the data row j = (u, r, v) at day t      iff  win_lo[t] <= j < win_hi[t]  and  lo <= t - row_day[j] < hi
//   the self-loop (u, n_rel_true, u) at t    iff  lo <= min(t, loop_window) < hi        (the lag the forward gives a self-loop)
//
// The chain of boolean products of rule_ground.hip with anchors for columns (rule_maps.h: the scratch layout cur / next / head / any,
// the seed and the count), as trule_ground.hip.  The anchors of a call are sorted by day and anchor_ptr [n_day + 1] holds the first
// anchor of every day, so day t owns the columns [ptr[t], ptr[t + 1]).  Because the windows are not monotone an edge does not move one
// column range: the hop walks the step's candidate days
//   data row j     t in [row_day[j] + lo, min(row_day[j] + hi, n_day)), each tested against its window
//   self-loop      the days that pass are one range: [lo, hi) where hi <= loop_window, [lo, n_day) where lo <= loop_window < hi
// and merges every run of consecutive passing days [a, b) into the one column range [ptr[a], ptr[b]), which it moves with the both-end
// masks and the integer atomicOr of move_range (rule_bits.h), as trule_hop_kernel does.  Merging changes no bit: the runs are
// disjoint and their union is the set of passing days.  Nothing bounds the candidate days from above but n_day: an "any" step or the open last bin tests every later day of
// the row (two loads from the window arrays, n_day entries each, per day).
//
//   fill    the whole scratch is zeroed by rg::zero_async
//   seed    bit j of cur[i][anchor_ent[j]]
//   head    one hop from the seed over the data rows (x, h, y): row j moves the columns of day row_day[j] - no window test, the fact on
//           the query day itself lies in no window - into `head`; the words that move are also ORed into any[i].  Never a self-loop.
//   hop l   the edges of relation body[i][l] under [lag_lo[i][l], lag_hi[i][l]) as above.  Then cur <-> next, the new next is zeroed
//   count   rule_count_kernel: body_pairs, hits, pca_body_pairs, head_pairs per rule
//
// Lanes.  The rule is blockIdx.y and a group of G lanes owns one edge: every lane of the group walks the edge's days (the loads are
// the same address for the group) and the group strides over the words of a run.  A workgroup has one step, so it picks G itself: the
// power of two >= the words a run can span, min(hi - lo, loop_window + 1) days at W / n_day words a day, plus one; at most the power
// of two >= W, at most 64.  With a few anchors per day that is G = 1 or 2 - 128 to 256 edges per workgroup pass - and the head pass,
// one day, takes G for one day.  A relation whose first edge is a self-loop (the identity relation holds nothing else) takes the
// row-wide G: its one range is most of the row.  A run wider than G is walked in strides of G, so every choice is correct.
// Measured against the row-wide group for every step (-DRG_XRULE_ONE_G: 2.2 - 2.4 times slower on narrow bins) and against one lane
// per edge (-DRG_XRULE_NARROW_G: 3.8 times slower where a day owns a dozen words), DESIGN.md section 5.
//
// Determinism.  OR and integer adds are order-independent: every count is exact and the same in every run, for every grid, every G and
// every cut of the anchors (in sorted order) and rules into calls.
//
// Bounds.  A relation id outside 0..n_rela_rows-1 is tested before any load and reads nothing; lag_lo >= lag_hi makes the step empty;
// an edge end or anchor entity outside 0..n_ent-1, a row index outside 0..n_data and a row_day outside 0..n_day-1 are skipped; the
// candidate days are formed in int64 and clamped to 0..n_day before any window entry is read; anchor_ptr entries are clamped to 0..S
// and a range with lo >= hi moves nothing.  The masks are move_range's (rule_bits.h: both shifts in 0..31).
#include "rule_maps.h"

namespace {

using namespace rgrule;

// one step of every rule: to[i][v] |= from[i][u] & columns(days the step admits the edge at) over the edges (u, v, j) of relation
// rel_of[i * stride] under the lags [lo_of[i * stride], hi_of[i * stride]).  lo_of NULL: the head pass - row j moves the columns of day
// row_day[j], self-loops move nothing - and `any` collects the bits that moved.  No barrier: a workgroup whose rule has no such
// relation, an empty lag range, or fewer edges than the grid covers, leaves.
__global__ __launch_bounds__(RT) void xrule_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht,
                                                       const int32_t* __restrict__ rel_tm, int32_t n_rela_rows, int32_t n_ent,
                                                       int32_t n_data, const int32_t* __restrict__ rel_of,
                                                       const int32_t* __restrict__ lo_of, const int32_t* __restrict__ hi_of,
                                                       int32_t stride, const int32_t* __restrict__ row_day,
                                                       const int32_t* __restrict__ win_lo, const int32_t* __restrict__ win_hi,
                                                       int32_t n_day, int32_t loop_window, const int32_t* __restrict__ anchor_ptr,
                                                       int32_t S, int32_t W, int32_t g_max, const uint32_t* __restrict__ from,
                                                       uint32_t* __restrict__ to, uint32_t* any) {
  const int64_t i = blockIdx.y;
  const int32_t r = rel_of[i * stride];
  if (r < 0 || r >= n_rela_rows) return;
  const bool is_head = lo_of == nullptr;
  const int64_t lag_lo = is_head ? 0 : lo_of[i * stride], lag_hi = is_head ? 1 : hi_of[i * stride];
  if (lag_lo >= lag_hi) return;
  const int64_t e0 = rel_ptr[r], e1 = rel_ptr[r + 1];
  if (e0 >= e1) return;
  // the lanes of an edge (the file comment): by the widest run of the step, row-wide for the identity relation
  int32_t g_shift = g_max;
#if defined(RG_XRULE_ONE_G)        // A/B builds (tools/build_variant.sh): the row-wide group for every step
#elif defined(RG_XRULE_NARROW_G)   // ... one lane per edge for every data-row step
  if (rel_tm[e0] != n_data) g_shift = 0;
#else
  if (rel_tm[e0] != n_data) {
    const int64_t days = std::min<int64_t>(lag_hi - lag_lo, (int64_t)loop_window + 1);
    const int64_t words = std::min<int64_t>(W, days * W / n_day + 1);
    g_shift = 0;
    while (g_shift < g_max && ((int64_t)1 << g_shift) < words) ++g_shift;
  }
#endif
  const Lanes ln = hop_lanes(g_shift);
  const int64_t base = i * n_ent * W;
  uint32_t* any_i = any ? any + i * W : nullptr;
  const auto ptr_at = [&](int32_t t) { return min(max(anchor_ptr[t], 0), S); };      // t in 0..n_day
  for (int64_t e = e0 + ln.first; e < e1; e += ln.step) {
    const int2 ht = rel_ht[e];
    const int32_t j = rel_tm[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent || (uint32_t)j > (uint32_t)n_data) continue;
    const uint32_t* __restrict__ src = from + base + (int64_t)ht.x * W;
    uint32_t* dst = to + base + (int64_t)ht.y * W;
    if (j == n_data) {                          // a self-loop: the days with lag_lo <= min(t, loop_window) < lag_hi are one range
      if (is_head || lag_lo > loop_window) continue;
      const int32_t a = (int32_t)std::min<int64_t>(std::max<int64_t>(lag_lo, 0), n_day);
      const int32_t b = lag_hi > loop_window ? n_day : (int32_t)std::min<int64_t>(lag_hi, n_day);      // (lag_hi <= 0: a >= b)
      if (a >= b) continue;
      const int32_t lo = ptr_at(a), hi = ptr_at(b);
      if (lo < hi) move_range(src, dst, any_i, lo, hi, ln);
      continue;
    }
    const int32_t d = row_day[j];
    if ((uint32_t)d >= (uint32_t)n_day) continue;
    if (is_head) {
      const int32_t lo = ptr_at(d), hi = ptr_at(d + 1);
      if (lo < hi) move_range(src, dst, any_i, lo, hi, ln);
      continue;
    }
    const int32_t t0 = (int32_t)std::min<int64_t>(std::max<int64_t>(d + lag_lo, 0), n_day);
    const int32_t t1 = (int32_t)std::min<int64_t>(std::max<int64_t>(d + lag_hi, 0), n_day);
    int32_t run = -1;                           // the first day of the current run of passing days
    for (int32_t t = t0; t < t1; ++t) {
      const bool pass = win_lo[t] <= j && j < win_hi[t];
      if (pass) {
        if (run < 0) run = t;
      } else if (run >= 0) {
        const int32_t lo = ptr_at(run), hi = ptr_at(t);
        if (lo < hi) move_range(src, dst, any_i, lo, hi, ln);
        run = -1;
      }
    }
    if (run >= 0) {
      const int32_t lo = ptr_at(run), hi = ptr_at(t1);
      if (lo < hi) move_range(src, dst, any_i, lo, hi, ln);
    }
  }
}

}  // namespace

extern "C" int rg_xrule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* lag_lo, const int32_t* lag_hi,
                               int32_t n_rules, int32_t n_hops, const int32_t* row_day, int32_t n_data, const int32_t* win_lo,
                               const int32_t* win_hi, int32_t n_day, int32_t loop_window, const int32_t* anchor_ent,
                               const int32_t* anchor_ptr, int32_t n_anchors, void* scratch, int64_t* counts, void* stream) {
  RG_CHECK(g, "rg_xrule_ground: NULL graph");
  RG_CHECK(n_data >= 0 && g->n_time != 0 && (int64_t)g->n_time == (int64_t)n_data + 1,
           "rg_xrule_ground: not the extrapolation layout (n_time=%d, n_data=%d: every edge's time field is its data row, n_time = n_data + 1)",
           g->n_time, n_data);
  RG_CHECK(g->rel_ptr && g->rel_ht && g->rel_tm, "rg_xrule_ground: the graph has no CSR by relation with edge times (rel_ptr / rel_tm is NULL)");
  if (ground_check("rg_xrule_ground", "anchors", n_rules, n_hops, n_anchors)) return 1;
  RG_CHECK(n_day >= 1, "rg_xrule_ground: n_day=%d", n_day);
  RG_CHECK(loop_window >= 0, "rg_xrule_ground: loop_window=%d", loop_window);
  if (n_rules == 0 || n_anchors == 0) return 0;
  const auto hop = [&](const Step& t) {
    const bool is_head = t.l < 0;      // the kernel knows the head pass by its NULL lags
    hipLaunchKernelGGL(xrule_hop_kernel, t.grid, dim3(RT), 0, t.s, g->rel_ptr, g->rel_ht, g->rel_tm, g->n_rela_rows, g->n_ent, n_data,
                       is_head ? head : body + t.l, is_head ? (const int32_t*)nullptr : lag_lo + t.l,
                       is_head ? (const int32_t*)nullptr : lag_hi + t.l, is_head ? 1 : n_hops, row_day, win_lo, win_hi, n_day, loop_window,
                       anchor_ptr, n_anchors, t.W, t.g_max, t.from, t.to, t.any);
  };
  return ground_chain("rg_xrule_ground", "anchors", g, n_rules, n_hops, anchor_ent, n_anchors,
                      head && body && lag_lo && lag_hi && (row_day || n_data == 0) && win_lo && win_hi && anchor_ent && anchor_ptr &&
                          scratch && counts,
                      scratch, counts, stream, hop);
}
