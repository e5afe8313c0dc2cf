// Application of weighted rules to queries (include/redgnn.h: rg_rule_apply): for every query (s, r) and entity y, which of the rules
// with head r connect s to y, folded in rule order into (best weight, its rule, product of the misses, number of rules that fired).
//
// The orientation of rule_ground.hip - entity-major bitmaps over the sources, "OR a source's word into a destination's" - with one
// difference: a rule's sources are only the queries of its head relation.  The host sorts the queries by relation (q_sub, q_row in
// sorted order, q_ptr by relation id), so rule i with head h has S_i = q_ptr[h + 1] - q_ptr[h] sources, W_i = ceil(S_i / 32) words
// per entity, and bit j of its bitmaps is the query at sorted position q_ptr[h] + j.  Its bitmaps are slabs of n_ent * W_i words at
// word slab[i] of two regions of the scratch:
//   cur, next : uint32 [n_words]       n_words = slab[n_rules]; bit j of word slab[i] + y * W_i + j / 32: source j reaches y under rule i
// A rule without queries has no slab and every kernel leaves it at once.  Word indices are int64 throughout.  The queries, the slabs,
// the seed and the aggregate live in rule_slabs.h, shared with trule_apply.hip (there q_ptr has n_time entries per relation, here one).
//
//   fill       the whole scratch is zeroed by rg::zero_async (a kernel: common.h says why no memset node)
//   seed       bit j of cur_i[q_sub[q_ptr[h] + j]]
//   hop l      for the edges (u, v) of relation body[i][l] and every word w: x = cur_i[u][w]; if x != 0: atomicOr(&next_i[v][w], x).
//              Then cur <-> next, and the new next is zeroed before the next hop
//   aggregate  one thread per cell (sorted position p, entity y), the lanes of a wave along y: the rules of the call whose head is p's
//              relation are found by binary search in `head` and visited in ascending order; where bit p - q_ptr[h] of cur_i[y] is set
//              the rule fires.  The four outputs of the cell, at [q_row[p]][y], are read when the first rule fires and stored once at the
//              end: a cell no rule of the call reaches costs no output traffic.  No atomics: a cell has one thread, and the calls that
//              carry the arrays from one range of rules to the next are ordered by the stream.
//
// The hop's inner loop is the whole-row move of rule_bits.h, the one rule_ground.hip's rule_hop_kernel runs (that kernel takes one W per
// call and collects `any`; here W, the slab and the lane group follow the rule): the rule is blockIdx.y, a group of G lanes owns one edge
// and runs along w, G the power of two >= W_i capped at 64, uniform within the workgroup.  OR is order-independent and the fold's
// order is the rule order, so every output is the same bit for bit in every run and however the rules are cut into calls.
//
// Bounds.  A relation id outside 0..n_rela_rows-1 is tested before any load and reads nothing; an edge end or subject outside
// 0..n_ent-1 and a q_row outside 0..batch-1 are skipped; q_ptr entries are clamped to 0..batch; a slab that does not lie inside
// 0..n_words is left out.  Whatever the arrays hold, nothing outside the graph, the scratch or the four outputs is touched.
#include "rule_slabs.h"

namespace {

using namespace rgapply;       // Queries, Slab, rule_slab, the seed and the aggregate (rule_slabs.h: shared with trule_apply.hip)

// step l of every rule: to_i[v] |= from_i[u] over the edges (u, v) of relation body[i][l].  No barrier: a workgroup whose rule has no
// query, no such relation, or fewer edges than the grid covers, leaves.
__global__ __launch_bounds__(RT) void apply_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht, Queries q,
                                                       const int32_t* __restrict__ head, const int32_t* __restrict__ body,
                                                       int32_t n_hops, int32_t l, const int64_t* __restrict__ slab, int32_t n_ent,
                                                       int64_t n_words, const uint32_t* __restrict__ from, uint32_t* __restrict__ to) {
  const int64_t i = blockIdx.y;
  const int32_t r = body[i * n_hops + l];
  if (r < 0 || r >= q.n_rela_rows) return;
  Slab sl;
  if (!rule_slab(q, head[i], slab, i, n_ent, n_words, &sl)) return;
  const int32_t W = sl.W;
  const int64_t e0 = rel_ptr[r], e1 = rel_ptr[r + 1];
  const Lanes ln = hop_lanes(group_shift(W));
  for (int64_t e = e0 + ln.first; e < e1; e += ln.step) {
    const int2 ht = rel_ht[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent) continue;
    move_row(from + sl.base + (int64_t)ht.x * W, to + sl.base + (int64_t)ht.y * W, nullptr, W, ln);
  }
}

}  // namespace

extern "C" size_t rg_rule_apply_scratch_bytes(int64_t n_words) {
  return rgapply::scratch_bytes(n_words);
}

extern "C" int rg_rule_apply(const rg_graph* g, const int32_t* head, const int32_t* body, const float* weight, const float* miss,
                             int32_t n_rules, int32_t n_hops, int32_t rule_base, const int32_t* q_sub, const int32_t* q_row,
                             const int32_t* q_ptr, int32_t batch, const int64_t* slab, int64_t n_words, void* scratch, int32_t phases,
                             float* best, float* surv, int32_t* best_rule, int32_t* fired, void* stream) {
  RG_CHECK(g, "rg_rule_apply: NULL graph");
  RG_CHECK(g->n_time == 0, "rg_rule_apply: temporal graph (n_time=%d): rules are grounded on static and inductive graphs only",
           g->n_time);
  RG_CHECK(g->rel_ptr && g->rel_ht, "rg_rule_apply: the graph has no CSR by relation (rel_ptr is NULL)");
  if (apply_check("rg_rule_apply", n_rules, n_hops, batch, phases, rule_base)) return 1;
  if (n_rules == 0 || batch == 0) return 0;
  const Queries q{q_sub, q_row, q_ptr, batch, g->n_rela_rows, 1};
  const Rules r{head, weight, miss, n_rules, n_hops, rule_base, slab, n_words, best, surv, best_rule, fired};
  const auto hop = [&](int32_t l, dim3 grid, hipStream_t s, const uint32_t* from, uint32_t* to) {
    hipLaunchKernelGGL(apply_hop_kernel, grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, q, head, body, n_hops, l, slab, g->n_ent, n_words,
                       from, to);
  };
  return apply_chain("rg_rule_apply", g, q, r,
                     head && body && weight && miss && q_sub && q_row && q_ptr && slab && scratch && best && surv && best_rule && fired,
                     scratch, phases, stream, hop);
}
