// What rule_apply.hip (static rules) and trule_apply.hip (temporal rules) share: the sorted queries, the per-rule slabs of the scratch,
// the seed kernel, the aggregate kernel - the one place where the fold over the firing rules is written - and the grid rule.  Both apply
// a rule as a chain of boolean products on entity-major bitmaps whose columns are only the queries of the rule's head relation.  The chain
// itself (apply_chain) is here too: a file adds its hop kernel - the step of its family around the moves of rule_bits.h - and the launch of it.
//
// The host sorts the queries (q_sub, q_row in sorted order) and gives q_ptr with `stride` entries per relation: relation h owns the
// sorted positions q_ptr[h * stride] .. q_ptr[(h + 1) * stride].  stride = 1: sorted by relation (rg_rule_apply); stride = n_time: sorted
// by (relation, time id), q_ptr[h * n_time + t] the first position of relation h whose time is >= t (rg_trule_apply).  Rule i with head
// h has S_i = p1 - p0 sources, W_i = ceil(S_i / 32) words per entity, and bit j of its bitmaps is the query at sorted position p0 + j.
// Its bitmaps are slabs of n_ent * W_i words at word slab[i] of two regions of the scratch:
//   cur, next : uint32 [n_words]       n_words = slab[n_rules]; bit j of word slab[i] + y * W_i + j / 32: source j reaches y under rule i
// A rule without queries has no slab and every kernel leaves it at once.  Word indices are int64 throughout.
#pragma once
#include "rule_bits.h"

namespace rgapply {
using namespace rgbits;      // the limits, grid_x, group_shift, the lane group and the moves, shared with rule_maps.h
namespace {

inline size_t region_bytes(int64_t n_words) { return rg::align_up((size_t)n_words * 4, RULE_ALIGN); }

struct Queries {
  const int32_t* sub;    // [batch] subjects in sorted order
  const int32_t* row;    // [batch] the caller's row of each sorted position
  const int32_t* ptr;    // [n_rela_rows * stride + 1] sorted positions by relation (and time id)
  int32_t batch, n_rela_rows;
  int32_t stride;        // entries of ptr per relation: 1, or n_time
};

struct Slab {
  int64_t base;          // first word
  int32_t p0, S, W;      // first sorted position, sources, words per entity
};

__device__ __forceinline__ int32_t clamp_pos(int32_t p, int32_t batch) { return p < 0 ? 0 : (p > batch ? batch : p); }

// the first sorted position of relation h (h in 0..n_rela_rows: the last one is the batch's end), clamped
__device__ __forceinline__ int32_t rel_pos(const Queries& q, int32_t h) { return clamp_pos(q.ptr[(int64_t)h * q.stride], q.batch); }

// the sources and slab of a rule with head h; false: no such relation, no query of it, or a slab outside the scratch
__device__ __forceinline__ bool rule_slab(const Queries& q, int32_t h, const int64_t* __restrict__ slab, int64_t i, int32_t n_ent,
                                          int64_t n_words, Slab* out) {
  if (h < 0 || h >= q.n_rela_rows) return false;
  const int32_t p0 = rel_pos(q, h), p1 = rel_pos(q, h + 1);
  if (p1 <= p0) return false;
  const int32_t W = (p1 - p0 + 31) >> 5;
  const int64_t base = slab[i];
  if (base < 0 || base > n_words || (int64_t)n_ent * W > n_words - base) return false;
  out->base = base; out->p0 = p0; out->S = p1 - p0; out->W = W;
  return true;
}

__global__ __launch_bounds__(RT) void apply_seed_kernel(Queries q, const int32_t* __restrict__ head, const int64_t* __restrict__ slab,
                                                        int32_t n_ent, int64_t n_words, uint32_t* __restrict__ cur) {
  const int64_t i = blockIdx.y;
  Slab sl;
  if (!rule_slab(q, head[i], slab, i, n_ent, n_words, &sl)) return;
  for (int32_t j = blockIdx.x * RT + threadIdx.x; j < sl.S; j += gridDim.x * RT) {
    const uint32_t s = (uint32_t)q.sub[sl.p0 + j];
    if (s < (uint32_t)n_ent) atomicOr(&cur[sl.base + (int64_t)s * sl.W + (j >> 5)], 1u << (j & 31));
  }
}

// blockIdx.y (strided) is the sorted position p, the threads run along y: p's relation, rule range and slabs are uniform in the
// workgroup, the four stores of a wave are 256 contiguous bytes each and so are its bitmap loads where W = 1.
__global__ __launch_bounds__(RT) void apply_aggregate_kernel(Queries q, const int32_t* __restrict__ head, const float* __restrict__ weight,
                                                             const float* __restrict__ miss, int32_t n_rules, int32_t rule_base,
                                                             const int64_t* __restrict__ slab, int32_t n_ent, int64_t n_words,
                                                             const uint32_t* __restrict__ cur, float* __restrict__ best,
                                                             float* __restrict__ surv, int32_t* __restrict__ best_rule,
                                                             int32_t* __restrict__ fired) {
  const int32_t y = blockIdx.x * RT + threadIdx.x;
  for (int32_t p = blockIdx.y; p < q.batch; p += gridDim.y) {
    const int32_t row = q.row[p];
    if ((uint32_t)row >= (uint32_t)q.batch) continue;
    int32_t lo = 0, hi = q.n_rela_rows;                   // the relation h that owns p: the last h whose first position is <= p
    while (hi - lo > 1) {
      const int32_t mid = (lo + hi) >> 1;
      if (rel_pos(q, mid) <= p) lo = mid; else hi = mid;
    }
    const int32_t h = lo;
    int32_t a = 0, b = n_rules;                           // first rule with head >= h
    while (a < b) {
      const int32_t mid = (a + b) >> 1;
      if (head[mid] < h) a = mid + 1; else b = mid;
    }
    if (a >= n_rules || head[a] != h || y >= n_ent) continue;
    const int64_t cell = (int64_t)row * n_ent + y;
    float c_best = 0.f, c_surv = 1.f;
    int32_t c_rule = -1, c_fired = 0;
    bool loaded = false;
    Slab sl;                                              // p0, S and W are the relation's: only the base changes with the rule
    if (!rule_slab(q, h, slab, a, n_ent, n_words, &sl)) continue;
    const int32_t j = p - sl.p0;
    if (j < 0 || j >= sl.S) continue;
    const int64_t word = (int64_t)y * sl.W + (j >> 5), span = (int64_t)n_ent * sl.W;
    for (int32_t i = a; i < n_rules && head[i] == h; ++i) {
      const int64_t base = slab[i];
      if (base < 0 || base > n_words || span > n_words - base) continue;
      const uint32_t x = cur[base + word];
      if (!((x >> (j & 31)) & 1u)) continue;
      if (!loaded) {
        c_best = best[cell]; c_surv = surv[cell]; c_rule = best_rule[cell]; c_fired = fired[cell];
        loaded = true;
      }
      const float w = weight[i];
      c_fired += 1;
      c_surv = __fmul_rn(c_surv, miss[i]);
      if (w > c_best) { c_best = w; c_rule = rule_base + i; }
    }
    if (loaded) {
      best[cell] = c_best; surv[cell] = c_surv; best_rule[cell] = c_rule; fired[cell] = c_fired;
    }
  }
}

// the scratch of both entry points: two regions of n_words words; 0 where n_words is outside 1..2^40
inline size_t scratch_bytes(int64_t n_words) {
  if (n_words < 1 || n_words > RULE_MAX_WORDS) return 0;
  return 2 * region_bytes(n_words);
}

// the argument checks both entry points (`fn`: its name) make alike; 0 = fine
inline int apply_check(const char* fn, int32_t n_rules, int32_t n_hops, int32_t batch, int32_t phases, int32_t rule_base) {
  if (check_rule_counts(fn, n_rules, n_hops)) return 1;
  RG_CHECK(batch >= 0, "%s: batch=%d", fn, batch);
  RG_CHECK(phases >= 1 && phases <= 3, "%s: phases=%d not in 1..3 (1: seed and hops, 2: aggregate)", fn, phases);
  RG_CHECK(rule_base >= 0 && rule_base <= INT32_MAX - RULE_MAX_RULES, "%s: rule_base=%d", fn, rule_base);
  return 0;
}

// what apply_chain needs beyond the queries: the rules of the call, their slabs and the four outputs
struct Rules {
  const int32_t* head;
  const float* weight;
  const float* miss;
  int32_t n_rules, n_hops, rule_base;
  const int64_t* slab;
  int64_t n_words;
  float* best;
  float* surv;
  int32_t* best_rule;
  int32_t* fired;
};

// An application call of n_rules >= 1 rules to batch >= 1 queries.  Phase 1: zero, seed, the hops with swap and re-zero; phase 2: the
// aggregate, which finds phase 1's result where the hops' swaps left it.  `all_given`: none of the entry point's pointers is NULL.
// hop(l, grid, s, from, to) launches step l of the family's hop kernel on `grid`, sized from the widest rule there can be.
template <class Hop>
int apply_chain(const char* fn, const rg_graph* g, const Queries& q, const Rules& r, bool all_given, void* scratch, int32_t phases,
                void* stream, Hop hop) {
  RG_CHECK(all_given, "%s: NULL argument", fn);
  const size_t bytes = scratch_bytes(r.n_words);
  RG_CHECK(bytes != 0, "%s: n_words=%lld is outside the bitmaps' range 1..2^40", fn, (long long)r.n_words);
  const hipStream_t s = (hipStream_t)stream;
  const int32_t n_ent = g->n_ent, n_rules = r.n_rules;
  uint32_t* cur = static_cast<uint32_t*>(scratch);
  uint32_t* next = reinterpret_cast<uint32_t*>(static_cast<unsigned char*>(scratch) + bytes / 2);
  const size_t map_bytes = (size_t)r.n_words * 4;

  if (phases & 1) {
    const int32_t g_shift = group_shift(rg::ceil_div(q.batch, 32));      // of the widest rule there can be: sizes the grid only
    const dim3 hop_grid(grid_x(g->n_fact, RT >> g_shift, n_rules), n_rules);
    if (rg::zero_async(scratch, bytes, s)) return 1;
    hipLaunchKernelGGL(apply_seed_kernel, dim3(grid_x(q.batch, RT, n_rules), n_rules), dim3(RT), 0, s, q, r.head, r.slab, n_ent,
                       r.n_words, cur);
    RG_LAUNCH_CHECK();
    for (int32_t l = 0; l < r.n_hops; ++l) {
      hop(l, hop_grid, s, cur, next);
      RG_LAUNCH_CHECK();
      std::swap(cur, next);
      if (l + 1 < r.n_hops && rg::zero_async(next, map_bytes, s)) return 1;
    }
  } else if (r.n_hops & 1) {
    std::swap(cur, next);                                 // where phase 1 left the result: one swap per hop
  }
  if (phases & 2) {
    const dim3 grid((unsigned)rg::ceil_div(n_ent, RT), (unsigned)std::min<int32_t>(q.batch, 65535));
    hipLaunchKernelGGL(apply_aggregate_kernel, grid, dim3(RT), 0, s, q, r.head, r.weight, r.miss, n_rules, r.rule_base, r.slab, n_ent,
                       r.n_words, cur, r.best, r.surv, r.best_rule, r.fired);
    RG_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace rgapply
