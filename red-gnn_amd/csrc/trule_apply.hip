// Application of weighted temporal rules to queries (include/redgnn.h: rg_trule_apply): for every query (s, r, t) and entity y, which
// of the rules with head r connect s to y under the directions of their steps against t, folded in rule order into (best weight, its
// rule, product of the misses, number of rules that fired).
//
// Two designs put together.  From rule_apply.hip the per-rule slabs (rule_slabs.h): a rule's columns are only the queries of its head
// relation, its two bitmaps are slabs of n_ent * W_i words at word slab[i] of the two regions of the scratch, and the seed and the
// aggregate - the fold - are that file's, taken from the header.  From trule_ground.hip the time ranges: the host sorts the queries
// stably by (relation, time id) and gives q_ptr int32 [n_rela_rows * n_time + 1], q_ptr[h * n_time + t] the first sorted position whose
// key is >= h * n_time + t.  Relation h owns p0 = q_ptr[h * n_time] .. p1 = q_ptr[(h + 1) * n_time], and inside a rule of head h an
// edge (u, v, tau) of the step's relation may move one contiguous column range (lo_t = q_ptr[h * n_time + tau] - p0, hi_t = q_ptr
// [h * n_time + tau + 1] - p0, S_i = p1 - p0):
//   past [hi_t, S_i)    now [lo_t, hi_t)    future [0, lo_t)    any [0, S_i)
// so a query's time is never loaded.  The hop reads only the words lo >> 5 .. (hi - 1) >> 5 of u's row, ANDs the first and the last
// with the range's mask (0xffffffff << (lo & 31) and 0xffffffff >> (31 - ((hi - 1) & 31)): both shifts lie in 0..31), skips what is
// zero and ORs the rest into v's row with an integer atomic.
//
//   fill       the whole scratch is zeroed by rg::zero_async
//   seed       apply_seed_kernel: bit j of cur_i[q_sub[p0 + j]]
//   hop l      the edges of relation body[i][l] (rows rel_ptr[r]..rel_ptr[r + 1] of rel_ht, times rel_tm) under direction dir[i][l], as
//              above.  Then cur <-> next, and the new next is zeroed before the next hop
//   aggregate  apply_aggregate_kernel with n_time entries of q_ptr per relation
//
// Lanes.  The rule is blockIdx.y and a group of G lanes owns one edge and runs along its words.  A workgroup has one rule, hence one
// W_i and one direction, and picks G itself: for a "now" step the power of two >= the mean width of a time id's range, W_i / n_time + 1
// words; for past, future and any, whose ranges average half the row or all of it, the power of two >= W_i, at most 64.  A range wider
// than G is walked in strides of G, so either choice is correct for every range (-DRG_TRULE_APPLY_ONE_G: the row-wide group for every
// direction, the A/B build of tools/build_variant.sh).  The grid is sized from the widest rule there can be.
//
// Determinism.  OR is order-independent and the fold's order is the rule order: every output is the same bit for bit in every run, for
// every grid and every G, and however the rules are cut into consecutive calls.
//
// Bounds.  A relation id outside 0..n_rela_rows-1 (head or step) is tested before any load and reads nothing; a direction outside 0..3
// makes the step empty; an edge end or subject outside 0..n_ent-1, an edge time outside 0..n_time-1 and a q_row outside 0..batch-1 are
// skipped; q_ptr is indexed in int64, its entries are clamped to 0..batch and the range to 0..S_i, and a range with lo >= hi moves
// nothing; a slab that does not lie inside 0..n_words is left out.  The bits of a slab's last word beyond S_i are never set by the seed
// and a hop only moves bits.  Whatever the arrays hold, nothing outside the graph, the scratch or the four outputs is touched.
#include "rule_slabs.h"

namespace {

using namespace rgapply;

// step l of every rule: to_i[v] |= from_i[u] & range(tau, d) over the edges (u, v, tau) of relation body[i][l] under direction
// dir[i][l].  No barrier: a workgroup whose rule has no query, no such relation or direction, or fewer edges than the grid covers, leaves.
__global__ __launch_bounds__(RT) void tapply_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht,
                                                        const int32_t* __restrict__ rel_tm, Queries q, int32_t n_time,
                                                        const int32_t* __restrict__ head, const int32_t* __restrict__ body,
                                                        const int32_t* __restrict__ dir, int32_t n_hops, int32_t l,
                                                        const int64_t* __restrict__ slab, int32_t n_ent, int64_t n_words,
                                                        const uint32_t* __restrict__ from, uint32_t* __restrict__ to) {
  const int64_t i = blockIdx.y;
  const int32_t r = body[i * n_hops + l];
  if (r < 0 || r >= q.n_rela_rows) return;
  const int32_t d = dir[i * n_hops + l];
  if (d < 0 || d > 3) return;
  const int32_t h = head[i];
  Slab sl;
  if (!rule_slab(q, h, slab, i, n_ent, n_words, &sl)) return;          // h is in 0..n_rela_rows-1 from here on
  const int32_t W = sl.W, S = sl.S;
#ifdef RG_TRULE_APPLY_ONE_G
  const int32_t g_shift = group_shift(W);
#else
  const int32_t g_shift = d == 1 ? group_shift(min(W, W / n_time + 1)) : group_shift(W);
#endif
  const int32_t* __restrict__ t_ptr = q.ptr + (int64_t)h * n_time;     // [n_time + 1] entries of q_ptr belong to h
  const int64_t e0 = rel_ptr[r], e1 = rel_ptr[r + 1];
  const Lanes ln = hop_lanes(g_shift);
  for (int64_t e = e0 + ln.first; e < e1; e += ln.step) {
    const int2 ht = rel_ht[e];
    const int32_t tau = rel_tm[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent || (uint32_t)tau >= (uint32_t)n_time) continue;
    int32_t lo = 0, hi = S;
    if (d != 3) {
      const int32_t c0 = min(max(clamp_pos(t_ptr[tau], q.batch) - sl.p0, 0), S);
      const int32_t c1 = min(max(clamp_pos(t_ptr[tau + 1], q.batch) - sl.p0, 0), S);
      if (d == 0) lo = c1;
      else if (d == 1) { lo = c0; hi = c1; }
      else hi = c0;
    }
    if (lo < hi) move_range(from + sl.base + (int64_t)ht.x * W, to + sl.base + (int64_t)ht.y * W, nullptr, lo, hi, ln);
  }
}

}  // namespace

extern "C" int rg_trule_apply(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* dir, const float* weight,
                              const float* miss, int32_t n_rules, int32_t n_hops, int32_t rule_base, const int32_t* q_sub,
                              const int32_t* q_row, const int32_t* q_ptr, int32_t batch, const int64_t* slab, int64_t n_words,
                              void* scratch, int32_t phases, float* best, float* surv, int32_t* best_rule, int32_t* fired,
                              void* stream) {
  RG_CHECK(g, "rg_trule_apply: NULL graph");
  RG_CHECK(g->n_time != 0, "rg_trule_apply: static graph (n_time=0): use rg_rule_apply");
  RG_CHECK(g->rel_ptr && g->rel_ht && g->rel_tm,
           "rg_trule_apply: the graph has no CSR by relation with edge times (rel_ptr / rel_ht / rel_tm is NULL)");
  if (apply_check("rg_trule_apply", n_rules, n_hops, batch, phases, rule_base)) return 1;
  if (n_rules == 0 || batch == 0) return 0;
  const Queries q{q_sub, q_row, q_ptr, batch, g->n_rela_rows, g->n_time};
  const Rules r{head, weight, miss, n_rules, n_hops, rule_base, slab, n_words, best, surv, best_rule, fired};
  const auto hop = [&](int32_t l, dim3 grid, hipStream_t s, const uint32_t* from, uint32_t* to) {
    hipLaunchKernelGGL(tapply_hop_kernel, grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, g->rel_tm, q, g->n_time, head, body, dir, n_hops, l,
                       slab, g->n_ent, n_words, from, to);
  };
  return apply_chain("rg_trule_apply", g, q, r,
                     head && body && dir && weight && miss && q_sub && q_row && q_ptr && slab && scratch && best && surv && best_rule &&
                         fired,
                     scratch, phases, stream, hop);
}
