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
__global__ __launch_bounds__(AT) void tapply_hop_kernel(const int32_t* __restrict__ rel_ptr, const int2* __restrict__ rel_ht,
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
  const int32_t G = 1 << g_shift, w0 = threadIdx.x & (G - 1);
  const int64_t per_block = AT >> g_shift;
  for (int64_t e = e0 + blockIdx.x * per_block + (threadIdx.x >> g_shift); e < e1; e += gridDim.x * per_block) {
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
    if (lo >= hi) continue;
    const int32_t w_lo = lo >> 5, w_hi = (hi - 1) >> 5;           // 0 <= w_lo <= w_hi < W: hi <= S
    const uint32_t m_lo = 0xffffffffu << (lo & 31), m_hi = 0xffffffffu >> (31 - ((hi - 1) & 31));
    const uint32_t* __restrict__ src = from + sl.base + (int64_t)ht.x * W;
    uint32_t* dst = to + sl.base + (int64_t)ht.y * W;
    for (int32_t w = w_lo + w0; w <= w_hi; w += G) {
      uint32_t x = src[w];
      if (w == w_lo) x &= m_lo;
      if (w == w_hi) x &= m_hi;
      if (x != 0) atomicOr(&dst[w], x);
    }
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
  RG_CHECK(n_rules >= 0 && n_rules <= APPLY_MAX_RULES, "rg_trule_apply: n_rules=%d not in 0..%d", n_rules, APPLY_MAX_RULES);
  RG_CHECK(n_hops >= 1 && n_hops <= APPLY_MAX_HOPS, "rg_trule_apply: n_hops=%d not in 1..%d", n_hops, APPLY_MAX_HOPS);
  RG_CHECK(batch >= 0, "rg_trule_apply: batch=%d", batch);
  RG_CHECK(phases >= 1 && phases <= 3, "rg_trule_apply: phases=%d not in 1..3 (1: seed and hops, 2: aggregate)", phases);
  RG_CHECK(rule_base >= 0 && rule_base <= INT32_MAX - APPLY_MAX_RULES, "rg_trule_apply: rule_base=%d", rule_base);
  if (n_rules == 0 || batch == 0) return 0;
  RG_CHECK(head && body && dir && weight && miss && q_sub && q_row && q_ptr && slab && scratch && best && surv && best_rule && fired,
           "rg_trule_apply: NULL argument");
  const size_t bytes = rgapply::scratch_bytes(n_words);
  RG_CHECK(bytes != 0, "rg_trule_apply: n_words=%lld is outside the bitmaps' range 1..2^40", (long long)n_words);
  const hipStream_t s = (hipStream_t)stream;
  const int32_t n_ent = g->n_ent, n_time = g->n_time;
  const Queries q{q_sub, q_row, q_ptr, batch, g->n_rela_rows, n_time};
  uint32_t* cur = static_cast<uint32_t*>(scratch);
  uint32_t* next = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(scratch) + bytes / 2);
  const size_t map_bytes = (size_t)n_words * 4;

  if (phases & 1) {
    const int32_t g_shift = group_shift(rg::ceil_div(batch, 32));      // of the widest rule there can be: sizes the grid only
    const dim3 hop_grid(grid_x(g->n_fact, AT >> g_shift, n_rules), n_rules);
    if (rg::zero_async(scratch, bytes, s)) return 1;
    hipLaunchKernelGGL(apply_seed_kernel, dim3(grid_x(batch, AT, n_rules), n_rules), dim3(AT), 0, s, q, head, slab, n_ent, n_words,
                       cur);
    RG_LAUNCH_CHECK();
    for (int32_t l = 0; l < n_hops; ++l) {
      hipLaunchKernelGGL(tapply_hop_kernel, hop_grid, dim3(AT), 0, s, g->rel_ptr, g->rel_ht, g->rel_tm, q, n_time, head, body, dir,
                         n_hops, l, slab, n_ent, n_words, cur, next);
      RG_LAUNCH_CHECK();
      std::swap(cur, next);
      if (l + 1 < n_hops && rg::zero_async(next, map_bytes, s)) return 1;
    }
  } else if (n_hops & 1) {
    std::swap(cur, next);                                 // where phase 1 left the result: one swap per hop
  }
  if (phases & 2) {
    const dim3 grid((unsigned)rg::ceil_div(n_ent, AT), (unsigned)std::min<int32_t>(batch, 65535));
    hipLaunchKernelGGL(apply_aggregate_kernel, grid, dim3(AT), 0, s, q, head, weight, miss, n_rules, rule_base, slab, n_ent, n_words,
                       cur, best, surv, best_rule, fired);
    RG_LAUNCH_CHECK();
  }
  return 0;
}
