// Grounding of mined rules on the whole graph (include/redgnn.h: rg_rule_ground): for every rule (head h, body r_1..r_L) and a set of
// sources X, how many pairs (x, y), x in X, the body connects, and how many of those the head connects too.
//
// A chain of boolean sparse products, one per step, on entity-major bitmaps over the sources - the frontier's orientation ("OR a
// source's word into a destination's").  A call covers n_r rules and S sources, W = ceil(S / 32) words per entity; the scratch holds
//   cur, next, head : uint32 [n_r][n_ent][W]      bit j of word (i, y, j / 32): source j reaches y under rule i
//   any             : uint32 [n_r][W]             bit j: source j has some fact of the rule's head relation
// Word indices are int64 throughout (n_r * n_ent * W passes 2^31 on a mid-sized graph with all entities as sources).
//
//   fill    the whole scratch is zeroed by rg::zero_async (a kernel: common.h says why no memset node)
//   seed    bit j of cur[i][sources[j]]
//   head    one hop from the seed with relation h into `head`; the words that move are also ORed into any[i]
//   hop l   for the edges (u, v) of relation r = body[i][l], rows rel_ptr[r]..rel_ptr[r + 1] of rel_ht, and every word w:
//           x = cur[i][u][w]; if x != 0: atomicOr(&next[i][v][w], x).  Then cur <-> next, and the new next is zeroed before the next hop
//   count   per rule, over all (y, w): body_pairs += popc(cur), hits += popc(cur & head), pca_body_pairs += popc(cur & any[w]),
//           head_pairs += popc(head); summed in the wave, then in the workgroup, then one 64-bit integer atomicAdd per workgroup
//
// Every launch covers all rules of the call (the rule is blockIdx.y).  In a hop a group of G lanes owns one edge and runs along w
// (G = 64 where W >= 64: a wave per edge, its lanes read 256 contiguous bytes of the source's row; G the power of two >= W below
// that, so a wave of narrow rows takes 64 / G edges at a time); the G lanes read the edge's 8 bytes from one address, which is one
// request.  Work per hop is |edges of r| * W words: no hop scans the graph.  OR and integer adds are order-independent: every count
// is exact and the same in every run, for every grid and every cut of the sources and rules into calls.
//
// Bounds.  A relation id outside 0..n_rela_rows-1 reads nothing (the rule then has no grounding); an edge end or a source outside
// 0..n_ent-1 is skipped.  The bits of the last word beyond the source count are never set by the seed, and a hop only moves bits.
#include "rule_maps.h"

namespace {

using namespace rgrule;      // the scratch layout, the seed and count kernels and the chain: shared with trule_ / xrule_ground.hip

// one step of every rule: to[i][v] |= from[i][u] over the edges (u, v) of relation rel_of[i * rel_stride]; `any` (or NULL) collects
// per word the bits that moved.  No barrier: a workgroup whose rule has no such relation, or fewer edges than the grid covers, leaves.
__global__ __launch_bounds__(RT) void rule_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht,
                                                      int32_t n_rela_rows, int32_t n_ent, const int32_t* __restrict__ rel_of,
                                                      int32_t rel_stride, int32_t W, int32_t g_shift,
                                                      const uint32_t* __restrict__ from, uint32_t* __restrict__ to, uint32_t* any) {
  const int64_t i = blockIdx.y;
  const int32_t r = rel_of[i * rel_stride];
  if (r < 0 || r >= n_rela_rows) return;
  const int64_t e0 = rel_ptr[r], e1 = rel_ptr[r + 1];
  const Lanes ln = hop_lanes(g_shift);
  const int64_t base = i * n_ent * W;
  uint32_t* any_i = any ? any + i * W : nullptr;
  for (int64_t e = e0 + ln.first; e < e1; e += ln.step) {
    const int2 ht = rel_ht[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent) continue;
    move_row(from + base + (int64_t)ht.x * W, to + base + (int64_t)ht.y * W, any_i, W, ln);
  }
}

}  // namespace

extern "C" size_t rg_rule_ground_scratch_bytes(int32_t n_ent, int32_t n_rules, int32_t n_sources) {
  return rgrule::scratch_bytes(n_ent, n_rules, n_sources);
}

extern "C" int rg_rule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, int32_t n_rules, int32_t n_hops,
                              const int32_t* sources, int32_t n_sources, void* scratch, int64_t* counts, void* stream) {
  RG_CHECK(g, "rg_rule_ground: NULL graph");
  RG_CHECK(g->n_time == 0, "rg_rule_ground: temporal graph (n_time=%d): rules are grounded on static and inductive graphs only",
           g->n_time);
  RG_CHECK(g->rel_ptr && g->rel_ht, "rg_rule_ground: the graph has no CSR by relation (rel_ptr is NULL)");
  if (ground_check("rg_rule_ground", "sources", n_rules, n_hops, n_sources)) return 1;
  if (n_rules == 0 || n_sources == 0) return 0;
  const auto hop = [&](const Step& t) {
    hipLaunchKernelGGL(rule_hop_kernel, t.grid, dim3(RT), 0, t.s, g->rel_ptr, g->rel_ht, g->n_rela_rows, g->n_ent,
                       t.l < 0 ? head : body + t.l, t.l < 0 ? 1 : n_hops, t.W, t.g_max, t.from, t.to, t.any);
  };
  return ground_chain("rg_rule_ground", "sources", g, n_rules, n_hops, sources, n_sources, head && body && sources && scratch && counts,
                      scratch, counts, stream, hop);
}
