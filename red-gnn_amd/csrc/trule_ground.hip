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
  const int32_t G = 1 << g_shift, w0 = threadIdx.x & (G - 1);
  const int64_t per_block = RT >> g_shift;
  const int64_t base = i * n_ent * W;
  uint32_t* any_i = any ? any + i * W : nullptr;
  for (int64_t e = e0 + blockIdx.x * per_block + (threadIdx.x >> g_shift); e < e1; e += gridDim.x * per_block) {
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
    if (lo >= hi) continue;
    const int32_t w_lo = lo >> 5, w_hi = (hi - 1) >> 5;           // 0 <= w_lo <= w_hi < W: hi <= S
    const uint32_t m_lo = 0xffffffffu << (lo & 31), m_hi = 0xffffffffu >> (31 - ((hi - 1) & 31));
    const uint32_t* __restrict__ src = from + base + (int64_t)ht.x * W;
    uint32_t* dst = to + base + (int64_t)ht.y * W;
    for (int32_t w = w_lo + w0; w <= w_hi; w += G) {
      uint32_t x = src[w];
      if (w == w_lo) x &= m_lo;
      if (w == w_hi) x &= m_hi;
      if (x != 0) {
        atomicOr(&dst[w], x);
        // the plain read may be stale: bits only ever appear, so a stale word costs an atomic and never drops one
        if (any_i && (any_i[w] & x) != x) atomicOr(&any_i[w], x);
      }
    }
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
  RG_CHECK(n_rules >= 0 && n_rules <= RULE_MAX_RULES, "rg_trule_ground: n_rules=%d not in 0..%d", n_rules, RULE_MAX_RULES);
  RG_CHECK(n_hops >= 1 && n_hops <= RULE_MAX_HOPS, "rg_trule_ground: n_hops=%d not in 1..%d", n_hops, RULE_MAX_HOPS);
  RG_CHECK(n_anchors >= 0, "rg_trule_ground: n_anchors=%d", n_anchors);
  if (n_rules == 0 || n_anchors == 0) return 0;
  RG_CHECK(head && body && dir && anchor_ent && anchor_ptr && scratch && counts, "rg_trule_ground: NULL argument");
  const size_t bytes = rg_trule_ground_scratch_bytes(g->n_ent, n_rules, n_anchors);
  RG_CHECK(bytes != 0, "rg_trule_ground: %d rules x %d entities x %d anchors is beyond the bitmaps' range", n_rules, g->n_ent,
           n_anchors);
  const hipStream_t s = (hipStream_t)stream;
  const int32_t n_ent = g->n_ent, n_time = g->n_time, S = n_anchors, W = (int32_t)rg::ceil_div(S, 32);
#ifdef RG_TRULE_ONE_G      // A/B build (tools/build_variant.sh): the row-wide group for every direction
  const int32_t g_wide = group_shift(W), g_now = g_wide;
#else
  const int32_t g_wide = group_shift(W), g_now = group_shift(std::min<int64_t>(W, W / n_time + 1));
#endif
  Maps m;
  carve(scratch, n_ent, n_rules, W, &m);
  const size_t map_bytes = (size_t)((int64_t)n_rules * n_ent * W) * 4;
  const dim3 hop_grid(grid_x(g->n_fact, RT >> g_wide, n_rules), n_rules);

  if (rg::zero_async(scratch, bytes, s)) return 1;
  hipLaunchKernelGGL(rule_seed_kernel, dim3(grid_x(S, RT, n_rules), n_rules), dim3(RT), 0, s, anchor_ent, S, n_ent, W, m.cur);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(trule_hop_kernel, hop_grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, g->rel_tm, g->n_rela_rows, n_ent, n_time, head,
                     (const int32_t*)nullptr, 1, anchor_ptr, S, W, g_now, g_wide, m.cur, m.head, m.any);
  RG_LAUNCH_CHECK();
  for (int32_t l = 0; l < n_hops; ++l) {
    hipLaunchKernelGGL(trule_hop_kernel, hop_grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, g->rel_tm, g->n_rela_rows, n_ent, n_time,
                       body + l, dir + l, n_hops, anchor_ptr, S, W, g_now, g_wide, m.cur, m.next, (uint32_t*)nullptr);
    RG_LAUNCH_CHECK();
    std::swap(m.cur, m.next);
    if (l + 1 < n_hops && rg::zero_async(m.next, map_bytes, s)) return 1;
  }
  hipLaunchKernelGGL(rule_count_kernel, dim3(grid_x((int64_t)n_ent * W, RT, n_rules), n_rules), dim3(RT), 0, s, n_ent, W, m.cur,
                     m.head, m.any, reinterpret_cast<unsigned long long*>(counts));
  RG_LAUNCH_CHECK();
  return 0;
}
