// What rule_apply.hip (static rules) and trule_apply.hip (temporal rules) share: the sorted queries, the per-rule slabs of the scratch,
// the seed kernel, the aggregate kernel - the one place where the fold over the firing rules is written - and the grid rule.  Both apply
// a rule as a chain of boolean products on entity-major bitmaps whose columns are only the queries of the rule's head relation; only the
// hop kernels differ, and each file keeps its own.
//
// The host sorts the queries (q_sub, q_row in sorted order) and gives q_ptr with `stride` entries per relation: relation h owns the
// sorted positions q_ptr[h * stride] .. q_ptr[(h + 1) * stride].  stride = 1: sorted by relation (rg_rule_apply); stride = n_time: sorted
// by (relation, time id), q_ptr[h * n_time + t] the first position of relation h whose time is >= t (rg_trule_apply).  Rule i with head
// h has S_i = p1 - p0 sources, W_i = ceil(S_i / 32) words per entity, and bit j of its bitmaps is the query at sorted position p0 + j.
// Its bitmaps are slabs of n_ent * W_i words at word slab[i] of two regions of the scratch:
//   cur, next : uint32 [n_words]       n_words = slab[n_rules]; bit j of word slab[i] + y * W_i + j / 32: source j reaches y under rule i
// A rule without queries has no slab and every kernel leaves it at once.  Word indices are int64 throughout.
#pragma once
#include <algorithm>

#include "common.h"

namespace rgapply {
namespace {

constexpr int AT = 256;                           // threads per workgroup
constexpr int APPLY_MAX_HOPS = 32;
constexpr int APPLY_MAX_RULES = 65535;            // the rule is blockIdx.y
constexpr size_t APPLY_ALIGN = 256;
constexpr int64_t APPLY_MAX_WORDS = (int64_t)1 << 40;   // per region (4 TiB): keeps every byte count far inside size_t

inline size_t region_bytes(int64_t n_words) { return rg::align_up((size_t)n_words * 4, APPLY_ALIGN); }

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

__global__ __launch_bounds__(AT) void apply_seed_kernel(Queries q, const int32_t* __restrict__ head, const int64_t* __restrict__ slab,
                                                        int32_t n_ent, int64_t n_words, uint32_t* __restrict__ cur) {
  const int64_t i = blockIdx.y;
  Slab sl;
  if (!rule_slab(q, head[i], slab, i, n_ent, n_words, &sl)) return;
  for (int32_t j = blockIdx.x * AT + threadIdx.x; j < sl.S; j += gridDim.x * AT) {
    const uint32_t s = (uint32_t)q.sub[sl.p0 + j];
    if (s < (uint32_t)n_ent) atomicOr(&cur[sl.base + (int64_t)s * sl.W + (j >> 5)], 1u << (j & 31));
  }
}

// blockIdx.y (strided) is the sorted position p, the threads run along y: p's relation, rule range and slabs are uniform in the
// workgroup, the four stores of a wave are 256 contiguous bytes each and so are its bitmap loads where W = 1.
__global__ __launch_bounds__(AT) void apply_aggregate_kernel(Queries q, const int32_t* __restrict__ head, const float* __restrict__ weight,
                                                             const float* __restrict__ miss, int32_t n_rules, int32_t rule_base,
                                                             const int64_t* __restrict__ slab, int32_t n_ent, int64_t n_words,
                                                             const uint32_t* __restrict__ cur, float* __restrict__ best,
                                                             float* __restrict__ surv, int32_t* __restrict__ best_rule,
                                                             int32_t* __restrict__ fired) {
  const int32_t y = blockIdx.x * AT + threadIdx.x;
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

// blocks along x for `items` units of work at `per_block` a pass, a few passes each, with the rules in y
inline unsigned grid_x(int64_t items, int64_t per_block, int32_t n_rules) {
  const int64_t want = rg::ceil_div(std::max<int64_t>(items, 1), per_block * 8);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(want, std::max<int64_t>(1, std::min<int64_t>(1024, 65536 / n_rules))));
}

// the power of two >= words, at most 64 (a wave), as a shift: the lanes that own one edge in a hop
__host__ __device__ __forceinline__ int32_t group_shift(int64_t words) {
  int32_t s = 0;
  while (s < 6 && ((int64_t)1 << s) < words) ++s;
  return s;
}

// the scratch of both entry points: two regions of n_words words; 0 where n_words is outside 1..2^40
inline size_t scratch_bytes(int64_t n_words) {
  if (n_words < 1 || n_words > APPLY_MAX_WORDS) return 0;
  return 2 * region_bytes(n_words);
}

}  // namespace
}  // namespace rgapply
