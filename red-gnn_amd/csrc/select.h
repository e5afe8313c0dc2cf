// Order keys of the top-k selections (topk.hip, segment_topk.hip) and the known-object index lookups of the per-segment kernels
// (segment_rank.hip, segment_topk.hip).
#pragma once
#include "common.h"

namespace {

// order-preserving 32-bit key of a score: NaN lowest, -0 == +0
__device__ __forceinline__ uint32_t key32(float x) {
  uint32_t u = __float_as_uint(x);
  if (x != x) return 0u;                         // NaN below -inf (whose key is 0x007FFFFF)
  if (u == 0x80000000u) u = 0u;                  // -0 == +0
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// unique 64-bit key of entity j (larger = better): score descending, then id ascending
__device__ __forceinline__ uint64_t order_key(uint32_t k32, uint32_t j) { return ((uint64_t)k32 << 32) | (uint64_t)(0xFFFFFFFFu - j); }

// [kb, ke) = the index's list of `key`; kb == ke when the index lacks it
__device__ __forceinline__ void key_range(const int64_t* __restrict__ keys, const int64_t* __restrict__ ptr, int64_t n_keys, int64_t key,
                                          int64_t* kb, int64_t* ke) {
  int64_t lo = 0, hi = n_keys;          // first index with keys[i] >= key
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1; else hi = mid;
  }
  *kb = *ke = 0;
  if (lo < n_keys && keys[lo] == key) {
    *kb = ptr[lo];
    *ke = max(ptr[lo + 1], *kb);
  }
}

// is x among list[0, n) (ascending)?
__device__ __forceinline__ bool list_has(const int32_t* list, int64_t n, int32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int32_t v = list[mid];
    if (v == x) return true;
    if (v < x) lo = mid + 1; else hi = mid;
  }
  return false;
}

}  // namespace
