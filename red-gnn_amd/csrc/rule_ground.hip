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
#include <algorithm>

#include "common.h"

namespace {

constexpr int RT = 256;                           // threads per workgroup
constexpr int RULE_MAX_HOPS = 32;
constexpr int RULE_MAX_RULES = 65535;             // the rule is blockIdx.y
constexpr size_t RULE_ALIGN = 256;
constexpr int64_t RULE_MAX_WORDS = (int64_t)1 << 40;   // per bitmap (4 TiB): keeps every byte count far inside size_t

struct Maps {
  uint32_t* cur;
  uint32_t* next;
  uint32_t* head;
  uint32_t* any;
};

inline size_t up(size_t x) { return (x + RULE_ALIGN - 1) / RULE_ALIGN * RULE_ALIGN; }

// slices of the scratch for n_r rules, W words per entity; returns the bytes used
size_t carve(void* scratch, int64_t n_ent, int64_t n_r, int64_t W, Maps* m) {
  unsigned char* p = static_cast<unsigned char*>(scratch);
  const size_t map = up((size_t)(n_r * n_ent * W) * 4);
  if (m) {
    m->cur = reinterpret_cast<uint32_t*>(p);
    m->next = reinterpret_cast<uint32_t*>(p + map);
    m->head = reinterpret_cast<uint32_t*>(p + 2 * map);
    m->any = reinterpret_cast<uint32_t*>(p + 3 * map);
  }
  return 3 * map + up((size_t)(n_r * W) * 4);
}

__global__ __launch_bounds__(RT) void rule_seed_kernel(const int32_t* __restrict__ sources, int32_t n_sources, int32_t n_ent, int32_t W,
                                                       uint32_t* __restrict__ cur) {
  const int64_t base = (int64_t)blockIdx.y * n_ent * W;
  for (int32_t j = blockIdx.x * RT + threadIdx.x; j < n_sources; j += gridDim.x * RT) {
    const uint32_t s = (uint32_t)sources[j];
    if (s < (uint32_t)n_ent) atomicOr(&cur[base + (int64_t)s * W + (j >> 5)], 1u << (j & 31));
  }
}

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
  const int32_t G = 1 << g_shift, w0 = threadIdx.x & (G - 1);
  const int64_t per_block = RT >> g_shift;
  const int64_t base = i * n_ent * W;
  uint32_t* any_i = any ? any + i * W : nullptr;
  for (int64_t e = e0 + blockIdx.x * per_block + (threadIdx.x >> g_shift); e < e1; e += gridDim.x * per_block) {
    const int2 ht = rel_ht[e];
    if ((uint32_t)ht.x >= (uint32_t)n_ent || (uint32_t)ht.y >= (uint32_t)n_ent) continue;
    const uint32_t* __restrict__ src = from + base + (int64_t)ht.x * W;
    uint32_t* dst = to + base + (int64_t)ht.y * W;
    for (int32_t w = w0; w < W; w += G) {
      const uint32_t x = src[w];
      if (x != 0) {
        atomicOr(&dst[w], x);
        // the plain read may be stale: bits only ever appear, so a stale word costs an atomic and never drops one
        if (any_i && (any_i[w] & x) != x) atomicOr(&any_i[w], x);
      }
    }
  }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(RT) void rule_count_kernel(int32_t n_ent, int32_t W, const uint32_t* __restrict__ cur,
                                                        const uint32_t* __restrict__ head, const uint32_t* __restrict__ any,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_part[RT / 64][4];
  const int64_t i = blockIdx.y, n = (int64_t)n_ent * W, stride = (int64_t)gridDim.x * RT;
  const uint32_t* __restrict__ c = cur + i * n;
  const uint32_t* __restrict__ h = head + i * n;
  const uint32_t* __restrict__ m = any + i * W;
  int64_t idx = (int64_t)blockIdx.x * RT + threadIdx.x;
  int32_t w = (int32_t)(idx % W);
  const int32_t w_step = (int32_t)(stride % W);
  unsigned long long body = 0, hits = 0, pca = 0, heads = 0;
  for (; idx < n; idx += stride) {
    const uint32_t x = c[idx], y = h[idx];
    if ((x | y) != 0) {
      body += __popc(x);
      hits += __popc(x & y);
      pca += __popc(x & m[w]);
      heads += __popc(y);
    }
    w += w_step;
    if (w >= W) w -= W;
  }
  body = wave_sum(body); hits = wave_sum(hits); pca = wave_sum(pca); heads = wave_sum(heads);
  if ((threadIdx.x & 63) == 0) {
    unsigned long long* p = s_part[threadIdx.x >> 6];
    p[0] = body; p[1] = hits; p[2] = pca; p[3] = heads;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    unsigned long long t = 0;
    for (int k = 0; k < RT / 64; ++k) t += s_part[k][threadIdx.x];
    if (t != 0) atomicAdd(&counts[i * 4 + threadIdx.x], t);
  }
}

// blocks along x for `items` units of work at `per_block` a pass, a few passes each, with the rules in y
unsigned grid_x(int64_t items, int64_t per_block, int32_t n_rules) {
  const int64_t want = rg::ceil_div(std::max<int64_t>(items, 1), per_block * 8);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, std::max<int64_t>(1, std::min<int64_t>(1024, 65536 / n_rules))));
}

}  // namespace

extern "C" size_t rg_rule_ground_scratch_bytes(int32_t n_ent, int32_t n_rules, int32_t n_sources) {
  if (n_ent < 1 || n_rules < 1 || n_rules > RULE_MAX_RULES || n_sources < 1) return 0;
  const int64_t W = rg::ceil_div(n_sources, 32);
  if ((int64_t)n_ent * W > RULE_MAX_WORDS / n_rules) return 0;
  return carve(nullptr, n_ent, n_rules, W, nullptr);
}

extern "C" int rg_rule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, int32_t n_rules, int32_t n_hops,
                              const int32_t* sources, int32_t n_sources, void* scratch, int64_t* counts, void* stream) {
  RG_CHECK(g, "rg_rule_ground: NULL graph");
  RG_CHECK(g->n_time == 0, "rg_rule_ground: temporal graph (n_time=%d): rules are grounded on static and inductive graphs only",
           g->n_time);
  RG_CHECK(g->rel_ptr && g->rel_ht, "rg_rule_ground: the graph has no CSR by relation (rel_ptr is NULL)");
  RG_CHECK(n_rules >= 0 && n_rules <= RULE_MAX_RULES, "rg_rule_ground: n_rules=%d not in 0..%d", n_rules, RULE_MAX_RULES);
  RG_CHECK(n_hops >= 1 && n_hops <= RULE_MAX_HOPS, "rg_rule_ground: n_hops=%d not in 1..%d", n_hops, RULE_MAX_HOPS);
  RG_CHECK(n_sources >= 0, "rg_rule_ground: n_sources=%d", n_sources);
  if (n_rules == 0 || n_sources == 0) return 0;
  RG_CHECK(head && body && sources && scratch && counts, "rg_rule_ground: NULL argument");
  const size_t bytes = rg_rule_ground_scratch_bytes(g->n_ent, n_rules, n_sources);
  RG_CHECK(bytes != 0, "rg_rule_ground: %d rules x %d entities x %d sources is beyond the bitmaps' range", n_rules, g->n_ent,
           n_sources);
  const hipStream_t s = (hipStream_t)stream;
  const int32_t n_ent = g->n_ent, W = (int32_t)rg::ceil_div(n_sources, 32);
  int32_t g_shift = 0;
  while (g_shift < 6 && (1 << g_shift) < W) ++g_shift;
  Maps m;
  carve(scratch, n_ent, n_rules, W, &m);
  const size_t map_bytes = (size_t)((int64_t)n_rules * n_ent * W) * 4;
  const dim3 hop_grid(grid_x(g->n_fact, RT >> g_shift, n_rules), n_rules);

  if (rg::zero_async(scratch, bytes, s)) return 1;
  hipLaunchKernelGGL(rule_seed_kernel, dim3(grid_x(n_sources, RT, n_rules), n_rules), dim3(RT), 0, s, sources, n_sources, n_ent, W,
                     m.cur);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(rule_hop_kernel, hop_grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, g->n_rela_rows, n_ent, head, 1, W, g_shift,
                     m.cur, m.head, m.any);
  RG_LAUNCH_CHECK();
  for (int32_t l = 0; l < n_hops; ++l) {
    hipLaunchKernelGGL(rule_hop_kernel, hop_grid, dim3(RT), 0, s, g->rel_ptr, g->rel_ht, g->n_rela_rows, n_ent, body + l, n_hops, W,
                       g_shift, m.cur, m.next, (uint32_t*)nullptr);
    RG_LAUNCH_CHECK();
    std::swap(m.cur, m.next);
    if (l + 1 < n_hops && rg::zero_async(m.next, map_bytes, s)) return 1;
  }
  hipLaunchKernelGGL(rule_count_kernel, dim3(grid_x((int64_t)n_ent * W, RT, n_rules), n_rules), dim3(RT), 0, s, n_ent, W, m.cur,
                     m.head, m.any, reinterpret_cast<unsigned long long*>(counts));
  RG_LAUNCH_CHECK();
  return 0;
}
