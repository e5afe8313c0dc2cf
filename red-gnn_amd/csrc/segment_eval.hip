// Loss term and filtered rank counts of the interpolation setting (include/redgnn.h: rg_segment_eval).
// Replaces the validation loop of Temporal/interpolation/main.py:125-183: F.softmax over the dense [B, n_ent] score matrix,
// F.nll_loss(log(p + 1e-12)), three torch.topk, a full argsort and one .nonzero().item() per query.  The interpolation score row is
// dense - an entity the query never reached scores exactly +0.0 and takes part in the softmax and in the ranking - but only the
// visited (query, entity) pairs carry information.  So one workgroup owns one query's segment of pairs, as in segment_rank.hip, and
// treats the row as "its pairs plus n_zero = n_ent - n_seg implicit zeros": the zeros enter the maximum, the sum and the counts
// arithmetically and the [B, n_ent] matrix is never built.
//
// With x the dense row, t the target and ts = x[t] (0 when t was not visited):
//   logp  = log(exp(ts - m) / Z + 1e-12),  m = max_e x[e],  Z = sum_seg exp(s_j - m) + n_zero exp(-m)
//   gt    = #{kept e: x[e] > ts},  eq = #{kept e != t: x[e] == ts}
// for three keep-sets: every entity; the entities not in the query's list of the first index; of the second - t always kept.  Of the
// implicit zeros a list L hides #{x in L, 0 <= x < n_ent, x != t} - #{pairs whose entity is in L, != t}.
//
// Maximum and sum are reduced in a fixed order (per-thread strided partials, wave shuffle, waves in index order) and the counters
// are integers: a query's results depend on its own segment and lists alone, bit for bit.
#include "select.h"

namespace {

constexpr int ET = 256;                 // threads per query (four wave64)
constexpr int EW = ET / 64;
constexpr int EVAL_LIST_LDS = 256;      // a known list of up to this many entities is searched in LDS, a longer one in memory

// first position of list[0, n) (ascending) whose entry is >= x
__device__ __forceinline__ int64_t list_lower(const int32_t* list, int64_t n, int32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (list[mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <typename PTR>
__global__ __launch_bounds__(ET) void segment_eval_kernel(
    const float* __restrict__ scores, const int32_t* __restrict__ ent, int64_t n_pairs, const PTR* __restrict__ seg_ptr,
    const int32_t* __restrict__ target, int32_t n_ent, const int64_t* __restrict__ key_a, const int64_t* __restrict__ a_keys,
    const int64_t* __restrict__ a_ptr, const int32_t* __restrict__ a_idx, int64_t n_a, const int64_t* __restrict__ key_b,
    const int64_t* __restrict__ b_keys, const int64_t* __restrict__ b_ptr, const int32_t* __restrict__ b_idx, int64_t n_b,
    float* __restrict__ logp, int32_t* __restrict__ count, int32_t* __restrict__ visited) {
  __shared__ int64_t s_rng[4];                      // [kb, ke) of the first list, then of the second
  __shared__ unsigned long long s_pos;              // position of the target's pair
  __shared__ int32_t s_list[2][EVAL_LIST_LDS];
  __shared__ int32_t s_inrange[2];                  // #{x in L, 0 <= x < n_ent, x != t} per list
  __shared__ float s_red[EW];
  __shared__ int s_cnt[8][EW];
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  // the segment, clamped to the pair arrays: nothing outside [0, n_pairs) is read whatever seg_ptr holds
  const int64_t b = min(max((int64_t)seg_ptr[q], (int64_t)0), n_pairs);
  const int64_t e = min(max((int64_t)seg_ptr[q + 1], b), n_pairs);
  const int32_t tgt = target[q];
  const int64_t n_zero = max((int64_t)n_ent - (e - b), (int64_t)0);

  if (tid == 0) s_pos = ~0ull;
  if (lane == 0 && w < 2) {                         // wave 0: the first index's key; wave 1: the second's
    int64_t kb = 0, ke = 0;
    if (w == 0) { if (n_a > 0) key_range(a_keys, a_ptr, n_a, key_a[q], &kb, &ke); }
    else if (n_b > 0) key_range(b_keys, b_ptr, n_b, key_b[q], &kb, &ke);
    s_rng[2 * w] = kb;
    s_rng[2 * w + 1] = ke;
  }
  __syncthreads();
  const int64_t kb0 = s_rng[0], n0 = s_rng[1] - kb0, kb1 = s_rng[2], n1 = s_rng[3] - kb1;
  const bool lds0 = n0 <= EVAL_LIST_LDS, lds1 = n1 <= EVAL_LIST_LDS;
  if (lds0) for (int i = tid; i < (int)n0; i += ET) s_list[0][i] = a_idx[kb0 + i];
  if (lds1) for (int i = tid; i < (int)n1; i += ET) s_list[1][i] = b_idx[kb1 + i];

  // pass 1: the target's pair and the maximum of the dense row (the zeros take part when there are any; fmaxf skips a NaN)
  float mx = n_zero > 0 ? 0.f : -INFINITY;
  for (int64_t j = b + tid; j < e; j += ET) {
    if (ent[j] == tgt) atomicMin(&s_pos, (unsigned long long)j);      // (entities are unique: one writer; else the first pair)
    mx = fmaxf(mx, scores[j]);
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_down(mx, o, 64));
  if (lane == 0) s_red[w] = mx;
  __syncthreads();                                  // (also: the lists are in LDS, s_pos is final)
  mx = s_red[0];
  for (int v = 1; v < EW; ++v) mx = fmaxf(mx, s_red[v]);
  const unsigned long long pos = s_pos;
  const bool seen = pos != ~0ull;
  const float ts = seen ? scores[pos] : 0.f;
  const bool zeros_count = 0.f >= ts;               // the implicit zeros change a count: every pair's list membership is needed
  const int32_t* l0 = lds0 ? s_list[0] : a_idx + kb0;
  const int32_t* l1 = lds1 ? s_list[1] : b_idx + kb1;
  if (lane == 0 && w < 2) {                         // the listed entities inside 0..n_ent-1 other than the target (lists ascend)
    const int32_t* l = w == 0 ? l0 : l1;
    const int64_t n = w == 0 ? n0 : n1;
    int64_t c = 0;
    if (n > 0) c = list_lower(l, n, n_ent) - list_lower(l, n, 0) - (tgt >= 0 && tgt < n_ent && list_has(l, n, tgt) ? 1 : 0);
    s_inrange[w] = (int32_t)min(c, (int64_t)0x7FFFFFFF);
  }
  __syncthreads();                                  // (s_red is read by everyone before pass 2 rewrites it)

  // pass 2: the sum, and gt / eq of all pairs, of those the first list keeps, of those the second keeps; c[6], c[7]: pairs (other
  // than the target's) that the first / second list names
  float sum = 0.f;
  int c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t j = b + tid; j < e; j += ET) {
    const float s = scores[j];
    sum += expf(s - mx);
    const bool ge = s >= ts;                        // lower scores and NaN change no count
    if (!ge && !zeros_count) continue;
    const int32_t x = ent[j];
    if (x == tgt) continue;                         // the target is always kept and never its own tie
    const int is_gt = s > ts, is_eq = s == ts;
    const bool in0 = n0 > 0 && list_has(l0, n0, x);
    const bool in1 = n1 > 0 && list_has(l1, n1, x);
    c[0] += is_gt; c[1] += is_eq;
    if (!in0) { c[2] += is_gt; c[3] += is_eq; } else c[6] += 1;
    if (!in1) { c[4] += is_gt; c[5] += is_eq; } else c[7] += 1;
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if (lane == 0) s_red[w] = sum;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int t = wave_sum(c[i]);
    if (lane == 0) s_cnt[i][w] = t;
  }
  __syncthreads();
  if (tid == 0) {
    sum = s_red[0];
    for (int v = 1; v < EW; ++v) sum += s_red[v];
    // the zeros' term only when there are zeros: on a full row whose maximum is below -88.7, expf(-mx) is +inf and 0 * inf is NaN
    const float Z = n_zero > 0 ? sum + (float)n_zero * expf(-mx) : sum;
    logp[q] = logf(expf(ts - mx) / Z + 1e-12f);
    int64_t t[8];
    for (int i = 0; i < 8; ++i) { t[i] = 0; for (int v = 0; v < EW; ++v) t[i] += s_cnt[i][v]; }
    // zeros other than the target's own; of those a list hides the entities it names that are not in the segment
    const int64_t zeros = n_zero - ((!seen && tgt >= 0 && tgt < n_ent) ? 1 : 0);
    int32_t* out = count + (int64_t)q * 6;
    for (int k = 0; k < 3; ++k) {
      const int64_t hidden = k == 0 ? 0 : max((int64_t)s_inrange[k - 1] - t[5 + k], (int64_t)0);
      const int64_t kept = max(zeros - hidden, (int64_t)0);
      out[2 * k] = (int32_t)(t[2 * k] + (0.f > ts ? kept : 0));
      out[2 * k + 1] = (int32_t)(t[2 * k + 1] + (0.f == ts ? kept : 0));
    }
    visited[q] = seen ? 1 : 0;
  }
}

template <typename PTR>
int launch(const float* scores, const int32_t* ent, int64_t n_pairs, const PTR* seg_ptr, const int32_t* target, int32_t batch, int32_t n_ent,
           const int64_t* key_a, const int64_t* a_keys, const int64_t* a_ptr, const int32_t* a_idx, int64_t n_a, const int64_t* key_b,
           const int64_t* b_keys, const int64_t* b_ptr, const int32_t* b_idx, int64_t n_b, float* logp, int32_t* count, int32_t* visited,
           hipStream_t s) {
  hipLaunchKernelGGL(segment_eval_kernel<PTR>, dim3(batch), dim3(ET), 0, s, scores, ent, n_pairs, seg_ptr, target, n_ent, key_a, a_keys,
                     a_ptr, a_idx, n_a, key_b, b_keys, b_ptr, b_idx, n_b, logp, count, visited);
  RG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int rg_segment_eval(const float* scores, const int32_t* ent, int64_t n_pairs, const void* seg_ptr, int32_t seg_ptr_is64,
                               const int32_t* target, int32_t batch, int32_t n_ent, const int64_t* key_a, const int64_t* a_keys,
                               const int64_t* a_ptr, const int32_t* a_idx, int64_t n_a, const int64_t* key_b, const int64_t* b_keys,
                               const int64_t* b_ptr, const int32_t* b_idx, int64_t n_b, float* logp_out, int32_t* count_out,
                               int32_t* visited_out, void* stream) {
  RG_CHECK(seg_ptr && target && logp_out && count_out && visited_out, "rg_segment_eval: NULL argument");
  RG_CHECK(batch > 0 && n_pairs >= 0, "rg_segment_eval: batch=%d n_pairs=%lld", batch, (long long)n_pairs);
  RG_CHECK(n_ent > 0, "rg_segment_eval: n_ent=%d", n_ent);
  RG_CHECK(n_pairs == 0 || (scores && ent), "rg_segment_eval: n_pairs=%lld with a NULL pair array", (long long)n_pairs);
  RG_CHECK(n_a >= 0 && n_b >= 0, "rg_segment_eval: n_keys=%lld / %lld", (long long)n_a, (long long)n_b);
  RG_CHECK(n_a == 0 || (a_keys && a_ptr && a_idx), "rg_segment_eval: n_keys=%lld with a NULL index array (first index)", (long long)n_a);
  RG_CHECK(n_b == 0 || (b_keys && b_ptr && b_idx), "rg_segment_eval: n_keys=%lld with a NULL index array (second index)", (long long)n_b);
  RG_CHECK((n_a == 0 || key_a) && (n_b == 0 || key_b), "rg_segment_eval: an index without per-query keys");
  const hipStream_t s = (hipStream_t)stream;
  if (seg_ptr_is64)
    return launch(scores, ent, n_pairs, (const int64_t*)seg_ptr, target, batch, n_ent, key_a, a_keys, a_ptr, a_idx, n_a, key_b, b_keys, b_ptr,
                  b_idx, n_b, logp_out, count_out, visited_out, s);
  return launch(scores, ent, n_pairs, (const int32_t*)seg_ptr, target, batch, n_ent, key_a, a_keys, a_ptr, a_idx, n_a, key_b, b_keys, b_ptr,
                b_idx, n_b, logp_out, count_out, visited_out, s);
}
