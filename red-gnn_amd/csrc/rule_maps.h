// What rule_ground.hip (static rules, columns = source entities) and trule_ground.hip (temporal rules, columns = anchors (entity,
// time id)) share: the scratch layout, the seed kernel, the counting kernel and the grid rule.  Both ground a rule as a chain of boolean
// products on entity-major bitmaps; a call covers n_r rules and S columns, W = ceil(S / 32) words per entity, and the scratch holds
//   cur, next, head : uint32 [n_r][n_ent][W]      bit j of word (i, y, j / 32): column j reaches y under rule i
//   any             : uint32 [n_r][W]             bit j: column j has some fact of the rule's head relation
// Word indices are int64 throughout (n_r * n_ent * W passes 2^31 on a mid-sized graph with all entities as sources).  The chain itself
// (ground_chain) is here too: a file adds its hop kernel - the step of its family around the moves of rule_bits.h - and the launch of it.
#pragma once
#include "rule_bits.h"

namespace rgrule {
using namespace rgbits;      // the limits, grid_x, group_shift, the lane group and the moves, shared with rule_slabs.h
namespace {

struct Maps {
  uint32_t* cur;
  uint32_t* next;
  uint32_t* head;
  uint32_t* any;
};

inline size_t up(size_t x) { return (x + RULE_ALIGN - 1) / RULE_ALIGN * RULE_ALIGN; }

// slices of the scratch for n_r rules, W words per entity; returns the bytes used
inline size_t carve(void* scratch, int64_t n_ent, int64_t n_r, int64_t W, Maps* m) {
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

// the bytes of a call's scratch; 0: an argument < 1, n_rules > RULE_MAX_RULES or more than RULE_MAX_WORDS words per bitmap
inline size_t scratch_bytes(int32_t n_ent, int32_t n_rules, int32_t n_cols) {
  if (n_ent < 1 || n_rules < 1 || n_rules > RULE_MAX_RULES || n_cols < 1) return 0;
  const int64_t W = rg::ceil_div(n_cols, 32);
  if ((int64_t)n_ent * W > RULE_MAX_WORDS / n_rules) return 0;
  return carve(nullptr, n_ent, n_rules, W, nullptr);
}

// bit j of cur[i][sources[j]] for every rule i; a source outside 0..n_ent-1 is skipped
__global__ __launch_bounds__(RT) void rule_seed_kernel(const int32_t* __restrict__ sources, int32_t n_sources, int32_t n_ent, int32_t W,
                                                       uint32_t* __restrict__ cur) {
  const int64_t base = (int64_t)blockIdx.y * n_ent * W;
  for (int32_t j = blockIdx.x * RT + threadIdx.x; j < n_sources; j += gridDim.x * RT) {
    const uint32_t s = (uint32_t)sources[j];
    if (s < (uint32_t)n_ent) atomicOr(&cur[base + (int64_t)s * W + (j >> 5)], 1u << (j & 31));
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

// the argument checks every grounding entry point (`fn`: its name) makes alike, its columns being `cols` ("sources", "anchors"); 0 = fine
inline int ground_check(const char* fn, const char* cols, int32_t n_rules, int32_t n_hops, int32_t n_cols) {
  if (check_rule_counts(fn, n_rules, n_hops)) return 1;
  RG_CHECK(n_cols >= 0, "%s: n_%s=%d", fn, cols, n_cols);
  return 0;
}

// what ground_chain hands a family's hop launch: one step of every rule of the call
struct Step {
  int32_t l;                 // the step, 0..n_hops-1; -1: the head pass, which collects `any`
  int32_t W, g_max;          // words per entity, and the row-wide lane group group_shift(W) the grid is sized for
  dim3 grid;
  hipStream_t s;
  const uint32_t* from;
  uint32_t* to;
  uint32_t* any;             // NULL in the body's steps
};

// A grounding call of n_rules >= 1 rules over S >= 1 columns, `col_ent` their entities: zero, seed, the head pass, the hops with swap
// and re-zero, count.  `all_given`: none of the entry point's pointers is NULL.  hop(step) launches the family's hop kernel.
template <class Hop>
int ground_chain(const char* fn, const char* cols, const rg_graph* g, int32_t n_rules, int32_t n_hops, const int32_t* col_ent, int32_t S,
                 bool all_given, void* scratch, int64_t* counts, void* stream, Hop hop) {
  RG_CHECK(all_given, "%s: NULL argument", fn);
  const size_t bytes = scratch_bytes(g->n_ent, n_rules, S);
  RG_CHECK(bytes != 0, "%s: %d rules x %d entities x %d %s is beyond the bitmaps' range", fn, n_rules, g->n_ent, S, cols);
  const hipStream_t s = (hipStream_t)stream;
  const int32_t n_ent = g->n_ent, W = (int32_t)rg::ceil_div(S, 32);
  const int32_t g_max = group_shift(W);
  Maps m;
  carve(scratch, n_ent, n_rules, W, &m);
  const size_t map_bytes = (size_t)((int64_t)n_rules * n_ent * W) * 4;
  const dim3 hop_grid(grid_x(g->n_fact, RT >> g_max, n_rules), n_rules);

  if (rg::zero_async(scratch, bytes, s)) return 1;
  hipLaunchKernelGGL(rule_seed_kernel, dim3(grid_x(S, RT, n_rules), n_rules), dim3(RT), 0, s, col_ent, S, n_ent, W, m.cur);
  RG_LAUNCH_CHECK();
  hop(Step{-1, W, g_max, hop_grid, s, m.cur, m.head, m.any});
  RG_LAUNCH_CHECK();
  for (int32_t l = 0; l < n_hops; ++l) {
    hop(Step{l, W, g_max, hop_grid, s, m.cur, m.next, nullptr});
    RG_LAUNCH_CHECK();
    std::swap(m.cur, m.next);
    if (l + 1 < n_hops && rg::zero_async(m.next, map_bytes, s)) return 1;
  }
  hipLaunchKernelGGL(rule_count_kernel, dim3(grid_x((int64_t)n_ent * W, RT, n_rules), n_rules), dim3(RT), 0, s, n_ent, W, m.cur,
                     m.head, m.any, reinterpret_cast<unsigned long long*>(counts));
  RG_LAUNCH_CHECK();
  return 0;
}

}  // namespace
}  // namespace rgrule
