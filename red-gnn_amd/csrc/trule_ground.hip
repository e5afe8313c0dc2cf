// Grounding of temporal rules on the whole quadruple graph (include/redgnn.h: rg_trule_ground): for every rule (head h, body
// (r_1, d_1)..(r_L, d_L)) and a set of anchors (x, t) - an entity and a query time id - how many pairs ((x, t), y) the body connects,
// and how many of those the head connects too.  d is the forward's direction of an edge of time id tau against the anchor's time t
// (dt = tau - t): 0 past (dt < 0), 1 now (dt == 0), 2 future (dt > 0); 3 = any time.  The head is a "now" step of relation h.
//
// The chain of boolean products of rule_ground.hip with anchors for columns (rule_maps.h: the scratch layout cur / next / head / any,
// the seed and the count).  The anchors of a call are j = 0..S-1, sorted by time id; anchor_ent[j] is their entity and anchor_ptr
// [n_time + 1] the first j whose time is >= tau (anchor_ptr[n_time] = S), so an anchor's time is never loaded: for an edge
// (u, v, tau) of the step's relation the anchors it may move are one contiguous column range,
//   past [ptr[tau + 1], S)    now [ptr[tau], ptr[tau + 1])    future [0, ptr[tau])    any [0, S)
// and the hop reads only the words lo >> 5 .. (hi - 1) >> 5 of u's row, ANDs the first and the last with the range's mask, and ORs
// what is left into v's row with an integer atomic.
//
//   fill    the whole scratch is zeroed by rg::zero_async
//   seed    bit j of cur[i][anchor_ent[j]]
//   head    one hop from the seed with relation h and direction "now" into `head`; the words that move are also ORed into any[i]
//   hop l   the edges of relation body[i][l] (rows rel_ptr[r]..rel_ptr[r + 1] of rel_ht, times rel_tm) under direction dir[i][l], as
//           above.  Then cur <-> next, and the new next is zeroed before the next hop
//   count   rule_count_kernel: body_pairs, hits, pca_body_pairs, head_pairs per rule, one 64-bit integer atomicAdd per workgroup
//
// Lanes.  Every launch covers all rules of the call (the rule is blockIdx.y), and a group of G lanes owns one edge and runs along its
// words.  A workgroup has one rule and hence one direction, so it picks G itself from two shifts the host passes: for a "now" step
// (and the head pass) the power of two >= the mean width of a time id's range, W / n_time + 1 words (with 8 192 anchors over 366 time
// ids that is G = 1: 256 edges per workgroup pass, where the row-wide G = 64 leaves 62 lanes of every wave without a word and was
// measured 3.8 times slower); for past, future and any, whose ranges average half the row or all of it, the power
// of two >= W, at most 64, as the static hop.  A range wider than G is walked in strides of G, so either choice is correct for
// every range.  Work per hop is |edges of r| * words in range.
//
// Determinism.  OR and integer adds are order-independent: every count is exact and the same in every run, for every grid, every G and
// every cut of the anchors (in sorted order) and rules into calls.
//
// Bounds.  A relation id outside 0..n_rela_rows-1 is tested before any load and reads nothing; a direction outside 0..3 makes the step
// empty; an edge end or anchor entity outside 0..n_ent-1 and an edge time outside 0..n_time-1 are skipped; anchor_ptr entries are
// clamped to 0..S and a range with lo >= hi moves nothing.  The masks are 0xffffffff << (lo & 31) and 0xffffffff >> (31 - ((hi - 1) &
// 31)): both shifts lie in 0..31 (a range that ends on a word boundary keeps its whole last word, a full word its 32 bits).  The bits of
// the last word beyond S are never set by the seed, and a hop only moves bits.
#include "rule_maps.h"

namespace {

using namespace rgrule;

// one step of every rule: to[i][v] |= from[i][u] & range(tau, d) over the edges (u, v, tau) of relation rel_of[i * stride] under
// direction dir_of[i * stride] (dir_of NULL: "now"); `any` (or NULL) collects per word the bits that moved.  No barrier: a workgroup
// whose rule has no such relation or direction, or fewer edges than the grid covers, leaves.
__global__ __launch_bounds__(RT) void trule_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht,
                                                       const int32_t* __restrict__ rel_tm, int32_t n_rela_rows, int32_t n_ent,
                                                       int32_t n_time, const int32_t* __restrict__ rel_of,
                                                       const int32_t* __restrict__ dir_of, int32_t stride,
                                                       const int32_t* __restrict__ anchor_ptr, int32_t S, int32_t W, int32_t g_now,
                                                       int32_t g_wide, const uint32_t* __restrict__ from, uint32_t* __restrict__ to,
                                                       uint32_t* any) {
  const int64_t i = blockIdx.y;
  const int32_t r = rel_of[i * stride];
  if (r < 0 || r >= n_rela_rows) return;
  const int32_t d = dir_of ? dir_of[i * stride] : 1;
  if (d < 0 || d > 3) return;
  const int64_t e0 = rel_ptr[r], e1 = rel_ptr[r + 1];
  const int32_t g_shift = d == 1 ? g_now : g_wide;
  const Lanes ln = hop_lanes(g_shift);
  const int64_t base = i * n_ent * W;
  uint32_t* any_i = any ? any + i * W : nullptr;
  for (int64_t e = e0 + ln.first; e < e1; e += ln.step) {
    const int2 ht = rel_ht[e];
    const int32_t tau = rel_tm[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent || (uint32_t)tau >= (uint32_t)n_time) continue;
    int32_t lo = 0, hi = S;
    if (d != 3) {
      const int32_t p0 = min(max(anchor_ptr[tau], 0), S), p1 = min(max(anchor_ptr[tau + 1], 0), S);
      if (d == 0) lo = p1;
      else if (d == 1) { lo = p0; hi = p1; }
      else hi = p0;
    }
    if (lo < hi) move_range(from + base + (int64_t)ht.x * W, to + base + (int64_t)ht.y * W, any_i, lo, hi, ln);
  }
}

}  // namespace

extern "C" size_t rg_trule_ground_scratch_bytes(int32_t n_ent, int32_t n_rules, int32_t n_anchors) {
  return rgrule::scratch_bytes(n_ent, n_rules, n_anchors);
}

extern "C" int rg_trule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* dir, int32_t n_rules,
                               int32_t n_hops, const int32_t* anchor_ent, const int32_t* anchor_ptr, int32_t n_anchors, void* scratch,
                               int64_t* counts, void* stream) {
  RG_CHECK(g, "rg_trule_ground: NULL graph");
  RG_CHECK(g->n_time != 0, "rg_trule_ground: static graph (n_time=0): use rg_rule_ground");
  RG_CHECK(g->rel_ptr && g->rel_ht && g->rel_tm, "rg_trule_ground: the graph has no CSR by relation with edge times (rel_ptr / rel_tm is NULL)");
  if (ground_check("rg_trule_ground", "anchors", n_rules, n_hops, n_anchors)) return 1;
  if (n_rules == 0 || n_anchors == 0) return 0;
  const auto hop = [&](const Step& t) {
#ifdef RG_TRULE_ONE_G      // A/B build (tools/build_variant.sh): the row-wide group for every direction
    const int32_t g_now = t.g_max;
#else
    const int32_t g_now = group_shift(std::min<int64_t>(t.W, t.W / g->n_time + 1));
#endif
    const bool is_head = t.l < 0;      // a "now" step: the kernel takes NULL directions for it
    hipLaunchKernelGGL(trule_hop_kernel, t.grid, dim3(RT), 0, t.s, g->rel_ptr, g->rel_ht, g->rel_tm, g->n_rela_rows, g->n_ent, g->n_time,
                       is_head ? head : body + t.l, is_head ? (const int32_t*)nullptr : dir + t.l, is_head ? 1 : n_hops, anchor_ptr,
                       n_anchors, t.W, g_now, t.g_max, t.from, t.to, t.any);
  };
  return ground_chain("rg_trule_ground", "anchors", g, n_rules, n_hops, anchor_ent, n_anchors,
                      head && body && dir && anchor_ent && anchor_ptr && scratch && counts, scratch, counts, stream, hop);
}
