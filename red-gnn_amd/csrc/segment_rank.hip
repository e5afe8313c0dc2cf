// Raw, filtered and time-filtered ranks of the extrapolation setting (include/redgnn.h: rg_segment_rank).
// Replaces segment_rank_fil of Temporal/extrapolation/segment.py:346-387: a Python loop over the queries of a batch with
// np.setdiff1d and a list comprehension per visited entity.  Here one workgroup owns one query's segment of the (query, entity)
// pairs and counts, with ts the score of the query's target,
//   rank = #{kept j: s_j > ts} + (#{kept j: s_j == ts} - 1) / 2 + 1
// three times: every pair kept; the pairs whose entity is not a known object of (s, p); of (s, p, t) - the target itself always
// kept.  The known objects come as the sorted CSR rg_topk reads (keys / ptr / idx); a key the index lacks filters nothing.
//
// Only integer counters, reduced in a fixed order: a query's result depends on its own segment and lists alone, bit for bit.
#include "select.h"

namespace {

constexpr int ST = 256;                 // threads per query (four wave64)
constexpr int SW = ST / 64;
constexpr int LIST_LDS = 256;           // a known-object list of up to this many entities is searched in LDS, a longer one in memory

__device__ __forceinline__ long long wave_sum(long long v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <typename PTR>
__global__ __launch_bounds__(ST) void segment_rank_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ ent, int64_t n_pairs, const PTR* __restrict__ seg_ptr,
    const int32_t* __restrict__ target, const int64_t* __restrict__ key_sp, const int64_t* __restrict__ sp_keys,
    const int64_t* __restrict__ sp_ptr, const int32_t* __restrict__ sp_idx, int64_t n_sp, const int64_t* __restrict__ key_spt,
    const int64_t* __restrict__ spt_keys, const int64_t* __restrict__ spt_ptr, const int32_t* __restrict__ spt_idx, int64_t n_spt,
    float* __restrict__ rank, float* __restrict__ rank_fil, float* __restrict__ rank_fil_t, int32_t* __restrict__ found) {
  __shared__ int64_t s_rng[4];                      // [kb, ke) of the (s, p) list, then of the (s, p, t) list
  __shared__ unsigned long long s_pos;              // position of the target's pair
  __shared__ int32_t s_list[2][LIST_LDS];
  __shared__ long long s_cnt[6][SW];
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // the segment, clamped to the pair arrays: nothing outside [0, n_pairs) is read whatever seg_ptr holds
  const int64_t b = min(max((int64_t)seg_ptr[q], (int64_t)0), n_pairs);
  const int64_t e = min(max((int64_t)seg_ptr[q + 1], b), n_pairs);
  const int32_t tgt = target[q];

  if (tid == 0) s_pos = ~0ull;
  if (lane == 0 && w < 2) {                         // wave 0: the (s, p) key; wave 1: the (s, p, t) key
    int64_t kb = 0, ke = 0;
    if (w == 0) { if (n_sp > 0) key_range(sp_keys, sp_ptr, n_sp, key_sp[q], &kb, &ke); }
    else if (n_spt > 0) key_range(spt_keys, spt_ptr, n_spt, key_spt[q], &kb, &ke);
    s_rng[2 * w] = kb;
    s_rng[2 * w + 1] = ke;
  }
  __syncthreads();
  const int64_t kb0 = s_rng[0], n0 = s_rng[1] - kb0, kb1 = s_rng[2], n1 = s_rng[3] - kb1;
  const bool lds0 = n0 <= LIST_LDS, lds1 = n1 <= LIST_LDS;
  if (lds0) for (int i = tid; i < (int)n0; i += ST) s_list[0][i] = sp_idx[kb0 + i];
  if (lds1) for (int i = tid; i < (int)n1; i += ST) s_list[1][i] = spt_idx[kb1 + i];
  for (int64_t j = b + tid; j < e; j += ST)
    if (ent[j] == tgt) atomicMin(&s_pos, (unsigned long long)j);      // (entities are unique: one writer; else the first pair)
  __syncthreads();
  const unsigned long long pos = s_pos;
  if (pos == ~0ull) {                               // the target was never reached (segment.py:383-386)
    if (tid == 0) { rank[q] = 1e9f; rank_fil[q] = 1e9f; rank_fil_t[q] = 1e9f; found[q] = 0; }
    return;
  }
  const float ts = scores[pos];

  int c[6] = {0, 0, 0, 0, 0, 0};                   // gt, eq of all pairs; of the (s, p)-filtered; of the (s, p, t)-filtered
  for (int64_t j = b + tid; j < e; j += ST) {
    const float s = scores[j];
    if (!(s >= ts)) continue;                       // lower scores and NaN change no count: no list search for them
    const int is_eq = s == ts, is_gt = 1 - is_eq;
    const int32_t x = ent[j];
    c[0] += is_gt; c[1] += is_eq;
    const bool own = x == tgt;
    const bool hid0 = !own && n0 > 0 && (lds0 ? list_has(s_list[0], n0, x) : list_has(sp_idx + kb0, n0, x));
    const bool hid1 = !own && n1 > 0 && (lds1 ? list_has(s_list[1], n1, x) : list_has(spt_idx + kb1, n1, x));
    if (!hid0) { c[2] += is_gt; c[3] += is_eq; }
    if (!hid1) { c[4] += is_gt; c[5] += is_eq; }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const long long t = wave_sum((long long)c[i]);
    if (lane == 0) s_cnt[i][w] = t;
  }
  __syncthreads();
  if (tid == 0) {
    long long t[6];
    for (int i = 0; i < 6; ++i) { t[i] = 0; for (int v = 0; v < SW; ++v) t[i] += s_cnt[i][v]; }
    // gt + (eq - 1)/2 + 1 = (2 gt + eq + 1)/2: one integer, one rounding
    rank[q] = (float)(2 * t[0] + t[1] + 1) * 0.5f;
    rank_fil[q] = (float)(2 * t[2] + t[3] + 1) * 0.5f;
    rank_fil_t[q] = (float)(2 * t[4] + t[5] + 1) * 0.5f;
    found[q] = 1;
  }
}

}  // namespace

extern "C" int rg_segment_rank(const float* scores, const int32_t* ent, int64_t n_pairs, const void* seg_ptr, int32_t seg_ptr_is64,
                               const int32_t* target, int32_t batch, const int64_t* key_sp, const int64_t* sp_keys, const int64_t* sp_ptr,
                               const int32_t* sp_idx, int64_t n_sp, const int64_t* key_spt, const int64_t* spt_keys,
                               const int64_t* spt_ptr, const int32_t* spt_idx, int64_t n_spt, float* rank_out, float* rank_fil_out,
                               float* rank_fil_t_out, int32_t* found_out, void* stream) {
  RG_CHECK(seg_ptr && target && rank_out && rank_fil_out && rank_fil_t_out && found_out, "rg_segment_rank: NULL argument");
  RG_CHECK(batch > 0 && n_pairs >= 0, "rg_segment_rank: batch=%d n_pairs=%lld", batch, (long long)n_pairs);
  RG_CHECK(n_pairs == 0 || (scores && ent), "rg_segment_rank: n_pairs=%lld with a NULL pair array", (long long)n_pairs);
  RG_CHECK(n_sp >= 0 && n_spt >= 0, "rg_segment_rank: n_keys=%lld / %lld", (long long)n_sp, (long long)n_spt);
  RG_CHECK(n_sp == 0 || (sp_keys && sp_ptr && sp_idx), "rg_segment_rank: n_keys=%lld with a NULL index array", (long long)n_sp);
  RG_CHECK(n_spt == 0 || (spt_keys && spt_ptr && spt_idx), "rg_segment_rank: n_keys=%lld with a NULL index array (time-dependent)",
           (long long)n_spt);
  RG_CHECK((n_sp == 0 || key_sp) && (n_spt == 0 || key_spt), "rg_segment_rank: an index without per-query keys");
  const hipStream_t s = (hipStream_t)stream;
  if (seg_ptr_is64)
    hipLaunchKernelGGL(segment_rank_kernel<int64_t>, dim3(batch), dim3(ST), 0, s, scores, ent, n_pairs, (const int64_t*)seg_ptr, target,
                       key_sp, sp_keys, sp_ptr, sp_idx, n_sp, key_spt, spt_keys, spt_ptr, spt_idx, n_spt, rank_out, rank_fil_out,
                       rank_fil_t_out, found_out);
  else
    hipLaunchKernelGGL(segment_rank_kernel<int32_t>, dim3(batch), dim3(ST), 0, s, scores, ent, n_pairs, (const int32_t*)seg_ptr, target,
                       key_sp, sp_keys, sp_ptr, sp_idx, n_sp, key_spt, spt_keys, spt_ptr, spt_idx, n_spt, rank_out, rank_fil_out,
                       rank_fil_t_out, found_out);
  RG_LAUNCH_CHECK();
  return 0;
}
