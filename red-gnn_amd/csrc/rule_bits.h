// What every rule kernel shares, grounding (rule_maps.h) and application (rule_slabs.h) alike: the limits of a call, the grid rule,
// the lane group of a hop and the two moves of a hop's inner loop.  A rule is a chain of boolean products on entity-major bitmaps,
// W words per entity; in a hop the rule is blockIdx.y, a group of G lanes (a power of two, at most a wave) owns one edge (u, v) of
// the step's relation and ORs the words of u's row - all of them, or those of one column range - into v's row.  What a family adds
// is its step: which edges, and which columns each may move.
#pragma once
#include <algorithm>

#include "common.h"

namespace rgbits {
namespace {

constexpr int RT = 256;                           // threads per workgroup
constexpr int RULE_MAX_HOPS = 32;
constexpr int RULE_MAX_RULES = 65535;             // the rule is blockIdx.y
constexpr size_t RULE_ALIGN = 256;
constexpr int64_t RULE_MAX_WORDS = (int64_t)1 << 40;   // per bitmap or region (4 TiB): keeps every byte count far inside size_t

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

// the two ranges every entry point (`fn`: its name) checks first; 0 = fine
inline int check_rule_counts(const char* fn, int32_t n_rules, int32_t n_hops) {
  RG_CHECK(n_rules >= 0 && n_rules <= RULE_MAX_RULES, "%s: n_rules=%d not in 0..%d", fn, n_rules, RULE_MAX_RULES);
  RG_CHECK(n_hops >= 1 && n_hops <= RULE_MAX_HOPS, "%s: n_hops=%d not in 1..%d", fn, n_hops, RULE_MAX_HOPS);
  return 0;
}

// a thread's place in a hop whose groups are 1 << g_shift lanes: a workgroup takes RT >> g_shift edges a pass
struct Lanes {
  int32_t G, w0;             // the lanes of an edge, and this lane's index among them
  int64_t first, step;       // this group's first edge, counted from the relation's first, and the grid's stride in edges
};

__device__ __forceinline__ Lanes hop_lanes(int32_t g_shift) {
  const int64_t per_block = RT >> g_shift;
  Lanes ln;
  ln.G = 1 << g_shift;
  ln.w0 = threadIdx.x & (ln.G - 1);
  ln.first = blockIdx.x * per_block + (threadIdx.x >> g_shift);
  ln.step = gridDim.x * per_block;
  return ln;
}

// dst[w] |= x by an integer atomic, skipped where x is 0; `any_i` (or NULL) collects per word the bits that moved
__device__ __forceinline__ void or_word(uint32_t* dst, uint32_t* any_i, int32_t w, uint32_t x) {
  if (x != 0) {
    atomicOr(&dst[w], x);
    // the plain read may be stale: bits only ever appear, so a stale word costs an atomic and never drops one
    if (any_i && (any_i[w] & x) != x) atomicOr(&any_i[w], x);
  }
}

// to[v] |= from[u], all W words of the row, by the lanes of a group.  Not move_range(0, S): that would put the two mask tests into
// the loop of the static hops.
__device__ __forceinline__ void move_row(const uint32_t* __restrict__ src, uint32_t* dst, uint32_t* any_i, int32_t W, const Lanes& ln) {
  for (int32_t w = ln.w0; w < W; w += ln.G) or_word(dst, any_i, w, src[w]);
}

// to[v] |= from[u] & columns [lo, hi), 0 <= lo < hi <= S, by the lanes of a group: only the words lo >> 5 .. (hi - 1) >> 5 are read,
// the first and the last ANDed with the range's mask.  Both shifts lie in 0..31: a range that ends on a word boundary keeps its whole
// last word, a full word its 32 bits.  A range wider than G words is walked in strides of G.
__device__ __forceinline__ void move_range(const uint32_t* __restrict__ src, uint32_t* dst, uint32_t* any_i, int32_t lo, int32_t hi,
                                           const Lanes& ln) {
  const int32_t w_lo = lo >> 5, w_hi = (hi - 1) >> 5;           // 0 <= w_lo <= w_hi < W: hi <= S
  const uint32_t m_lo = 0xffffffffu << (lo & 31), m_hi = 0xffffffffu >> (31 - ((hi - 1) & 31));
  for (int32_t w = w_lo + ln.w0; w <= w_hi; w += ln.G) {
    uint32_t x = src[w];
    if (w == w_lo) x &= m_lo;
    if (w == w_hi) x &= m_hi;
    or_word(dst, any_i, w, x);
  }
}

}  // namespace
}  // namespace rgbits
