// Filtered top-k of every query's segment of visited (query, entity) pairs (include/redgnn.h: rg_segment_topk): what rg_topk is for a
// dense score row, in rg_segment_rank's layout - the forecasts of the extrapolation model, which ranks a query among the entities its
// window reaches only.
//
// One workgroup per query.  Pair i of the segment gets the unique order key of topk.hip,
//   K(i) = key32(score_i) << 32 | (0xFFFFFFFF - ent_i)        (larger = better; NaN lowest, -0 == +0)
// and is kept unless ent_i is in the query's known-object list (binary search; a list of up to SEG_LIST_LDS = 256 entities is
// searched in LDS, a longer one in memory).  The same 8-bit radix select as rg_topk narrows the prefix of the k-th largest kept key
// (usually 2-3 passes; heavy ties go on into the id digits), the selected pairs are gathered into LDS with their positions, sorted
// by a bitonic sort and written out.  Segments of up to SEG_STAGE_MAX = 24576 pairs keep key32 and the kept flag in LDS after the
// first pass; longer ones re-read scores and entities and repeat the search on every pass.
//
// prob_out is the per-query softmax over ALL pairs of the segment (scatter_softmax of model_cuda_new_embedding.py:248), its maximum
// and sum reduced in a fixed order: per-thread strided partials, wave shuffle, then the waves in index order.  The selection uses
// integer LDS atomics only.  A query's results depend on its own segment and list alone, bit for bit.
#include "select.h"

namespace {

constexpr int QT = 512;                 // threads per query
constexpr int QW = QT / 64;             // waves
constexpr int SEG_TOPK_MAX = 1024;
constexpr int64_t SEG_STAGE_MAX = 24576;     // 120 KiB of key32 + flags, 21 KiB of histograms, candidates and list <= 160 KiB
constexpr int SEG_LIST_LDS = 256;

// layout of the dynamic LDS: [sub-histograms int32 QW x 256][candidate keys uint64 K_MAX][their positions uint32 K_MAX]
// [known list int32 SEG_LIST_LDS][key32 uint32 stage][kept uint8 stage]
constexpr size_t LDS_HIST = (size_t)QW * 256 * 4, LDS_CAND = (size_t)SEG_TOPK_MAX * 8, LDS_POS = (size_t)SEG_TOPK_MAX * 4;
constexpr size_t LDS_LIST = (size_t)SEG_LIST_LDS * 4;
constexpr size_t LDS_FIXED = LDS_HIST + LDS_CAND + LDS_POS + LDS_LIST;

template <typename PTR>
__global__ __launch_bounds__(QT) void segment_topk_kernel(const float* __restrict__ scores, const int32_t* __restrict__ ent,
                                                           int64_t n_pairs, const PTR* __restrict__ seg_ptr, int32_t k,
                                                           const int64_t* __restrict__ q_key, const int64_t* __restrict__ known_keys,
                                                           const int64_t* __restrict__ known_ptr, const int32_t* __restrict__ known_idx,
                                                           int64_t n_keys, uint32_t stage_cap, int32_t* __restrict__ idx_out,
                                                           float* __restrict__ score_out, float* __restrict__ prob_out) {
  extern __shared__ __align__(16) unsigned char lds[];
  int32_t* sub = reinterpret_cast<int32_t*>(lds);                                            // [QW][256]
  uint64_t* cand = reinterpret_cast<uint64_t*>(lds + LDS_HIST);                                // [SEG_TOPK_MAX]
  uint32_t* cpos = reinterpret_cast<uint32_t*>(lds + LDS_HIST + LDS_CAND);                     // [SEG_TOPK_MAX]
  int32_t* s_list = reinterpret_cast<int32_t*>(lds + LDS_HIST + LDS_CAND + LDS_POS);           // [SEG_LIST_LDS]
  uint32_t* s_key = reinterpret_cast<uint32_t*>(lds + LDS_FIXED);                              // [stage_cap]
  uint8_t* s_keep = reinterpret_cast<uint8_t*>(s_key + stage_cap);                             // [stage_cap]
  __shared__ int64_t s_rng[2];          // [kb, ke) of the query's known list
  __shared__ int32_t ctrl[16];
  __shared__ float s_red[QW];

  const int64_t q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int32_t* my_sub = sub + w * 256;
  // the segment, clamped to the pair arrays: nothing outside [0, n_pairs) is read whatever seg_ptr holds
  const int64_t b = min(max((int64_t)seg_ptr[q], (int64_t)0), n_pairs);
  const int64_t e = min(max((int64_t)seg_ptr[q + 1], b), n_pairs);
  const uint32_t len = (uint32_t)min(e - b, (int64_t)0x7FFFFFFF);
  const bool staged = len <= stage_cap;
  const float* __restrict__ sc = scores + b;
  const int32_t* __restrict__ en = ent + b;

  for (int i = tid; i < QW * 256; i += QT) sub[i] = 0;
  if (tid == 0) {
    int64_t kb = 0, ke = 0;
    if (n_keys > 0) key_range(known_keys, known_ptr, n_keys, q_key[q], &kb, &ke);
    s_rng[0] = kb;
    s_rng[1] = ke;
  }
  __syncthreads();
  const int64_t kb = s_rng[0], n_list = s_rng[1] - kb;
  const bool list_lds = n_list <= SEG_LIST_LDS;
  if (list_lds) for (int i = tid; i < (int)n_list; i += QT) s_list[i] = known_idx[kb + i];

  // softmax statistics over every pair of the segment, excluded ones included; a NaN score makes the sum NaN
  float mx = -INFINITY, sum = 0.f;
  if (prob_out) {
    for (uint32_t i = tid; i < len; i += QT) mx = fmaxf(mx, sc[i]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_down(mx, o, 64));
    if (lane == 0) s_red[w] = mx;
    __syncthreads();
    mx = s_red[0];
    for (int v = 1; v < QW; ++v) mx = fmaxf(mx, s_red[v]);
    __syncthreads();
    for (uint32_t i = tid; i < len; i += QT) sum += expf(sc[i] - mx);
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if (lane == 0) s_red[w] = sum;
    __syncthreads();
    sum = s_red[0];
    for (int v = 1; v < QW; ++v) sum += s_red[v];
  }
  __syncthreads();                      // (the list is in LDS)

  // order key of pair i and whether it is kept; `fresh`: from memory (and into LDS when staged), else from LDS
  auto pair_key = [&](uint32_t i, bool fresh, uint64_t* K) -> bool {
    const int32_t x = en[i];
    uint32_t k32;
    bool keep;
    if (fresh) {
      k32 = key32(sc[i]);
      keep = !(n_list > 0 && (list_lds ? list_has(s_list, n_list, x) : list_has(known_idx + kb, n_list, x)));
      if (staged) { s_key[i] = k32; s_keep[i] = keep; }
    } else {
      k32 = s_key[i];
      keep = s_keep[i] != 0;
    }
    *K = order_key(k32, (uint32_t)x);
    return keep;
  };

  int32_t need = k;
  uint64_t prefix = 0;
  int plen = 0;                    // bits of the selected prefix; 0 = every kept pair is selected
  bool done = false;
  for (int d = 0; d < 8 && !done; ++d) {
    const int shift = 56 - 8 * d;
    const int hs = 64 - plen;      // prefix test: (K >> hs) == prefix (plen > 0)
    for (uint32_t i = tid; i < len; i += QT) {
      uint64_t K;
      if (!pair_key(i, !staged || d == 0, &K)) continue;
      if (plen == 0 || (K >> hs) == prefix) atomicAdd(&my_sub[(K >> shift) & 0xFF], 1);
    }
    __syncthreads();
    if (w == 0) {
      // lane l holds bins 255-4l .. 252-4l (descending), reads and clears them; an inclusive scan over lanes finds the bin of the
      // need-th largest key
      int c[4], s = 0;
      for (int i = 0; i < 4; ++i) {
        const int bin = 255 - 4 * lane - i;
        int t = 0;
        for (int v = 0; v < QW; ++v) { t += sub[v * 256 + bin]; sub[v * 256 + bin] = 0; }
        c[i] = t;
        s += t;
      }
      int incl = s;
      for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(incl, o, 64);
        if (lane >= o) incl += y;
      }
      const int total = __shfl(incl, 63, 64);
      const int excl = incl - s;
      if (d == 0 && total <= need) {
        if (lane == 0) { ctrl[4] = 1; ctrl[6] = total; }                 // no more than k are kept: take them all
      } else {
        const uint64_t m = __ballot(excl < need && need <= incl);
        const int at = m ? __ffsll((long long)m) - 1 : -1;
        if (at < 0) {
          if (lane == 0) { ctrl[4] = 1; ctrl[6] = need; }                // (unreachable: the counts of a pass are consistent)
        } else if (lane == at) {
          int above = excl, i = 0;
          while (i < 3 && need > above + c[i]) { above += c[i]; ++i; }
          const int rem = need - above;
          ctrl[4] = 0; ctrl[5] = 255 - 4 * lane - i; ctrl[6] = rem; ctrl[7] = c[i] == rem;
        }
      }
    }
    __syncthreads();
    need = ctrl[6];
    if (ctrl[4]) {                   // everything that is kept
      plen = 0;
      prefix = 0;
      done = true;
    } else {
      prefix = (prefix << 8) | (uint64_t)ctrl[5];
      plen += 8;
      done = ctrl[7] != 0;
    }                                // (the next pass rewrites ctrl only after its histogram's barrier)
  }

  // gather the selected pairs (exactly min(k, #kept) of them when the entities are unique; never more than SEG_TOPK_MAX are stored)
  if (tid == 0) ctrl[8] = 0;
  __syncthreads();
  const int hs = 64 - plen;
  for (uint32_t i = tid; i < len; i += QT) {
    uint64_t K;
    if (!pair_key(i, !staged, &K)) continue;
    if (plen == 0 || (K >> hs) >= prefix) {
      const int pos = atomicAdd(&ctrl[8], 1);
      if (pos < SEG_TOPK_MAX) { cand[pos] = K; cpos[pos] = i; }
    }
  }
  __syncthreads();
  const int n = min(min(ctrl[8], k), SEG_TOPK_MAX);
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += QT) { cand[i] = 0; cpos[i] = 0; }     // below every real key (never read back: i >= n)
  __syncthreads();
  // bitonic sort by key, descending, the positions moving with their keys
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += QT) {
        const int i = 2 * t - (t & (stride - 1));
        const int jx = i + stride;
        const bool desc = (i & size) == 0;
        const uint64_t a = cand[i], c = cand[jx];
        if ((a < c) == desc) {
          const uint32_t pa = cpos[i];
          cand[i] = c; cand[jx] = a;
          cpos[i] = cpos[jx]; cpos[jx] = pa;
        }
      }
      __syncthreads();
    }
  }
  int32_t* irow = idx_out + q * (int64_t)k;
  float* srow = score_out + q * (int64_t)k;
  float* prow = prob_out ? prob_out + q * (int64_t)k : nullptr;
  for (int i = tid; i < k; i += QT) {
    if (i < n) {
      const float s = sc[cpos[i]];
      irow[i] = (int32_t)(0xFFFFFFFFu - (uint32_t)cand[i]);
      srow[i] = s;
      if (prow) prow[i] = expf(s - mx) / sum;
    } else {
      irow[i] = -1;
      srow[i] = -INFINITY;
      if (prow) prow[i] = 0.f;
    }
  }
}

template <typename PTR>
int launch(const float* scores, const int32_t* ent, int64_t n_pairs, const PTR* seg_ptr, int32_t batch, int32_t k, const int64_t* q_key,
           const int64_t* known_keys, const int64_t* known_ptr, const int32_t* known_idx, int64_t n_keys, int32_t* idx_out,
           float* score_out, float* prob_out, hipStream_t s) {
  const uint32_t stage_cap = (uint32_t)min(n_pairs, SEG_STAGE_MAX);        // no segment is longer than n_pairs
  const size_t lds = LDS_FIXED + rg::align_up((size_t)stage_cap * 5, 16);
  if (lds > 64 * 1024)
    RG_HIP(hipFuncSetAttribute((const void*)segment_topk_kernel<PTR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(segment_topk_kernel<PTR>, dim3(batch), dim3(QT), lds, s, scores, ent, n_pairs, seg_ptr, k, q_key, known_keys,
                     known_ptr, known_idx, n_keys, stage_cap, idx_out, score_out, prob_out);
  RG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int rg_segment_topk(const float* scores, const int32_t* ent, int64_t n_pairs, const void* seg_ptr, int32_t seg_ptr_is64,
                               int32_t batch, int32_t k, const int64_t* q_key, const int64_t* known_keys, const int64_t* known_ptr,
                               const int32_t* known_idx, int64_t n_keys, int32_t* idx_out, float* score_out, float* prob_out,
                               void* stream) {
  RG_CHECK(seg_ptr && idx_out && score_out, "rg_segment_topk: NULL argument");
  RG_CHECK(batch > 0 && n_pairs >= 0, "rg_segment_topk: batch=%d n_pairs=%lld", batch, (long long)n_pairs);
  RG_CHECK(n_pairs == 0 || (scores && ent), "rg_segment_topk: n_pairs=%lld with a NULL pair array", (long long)n_pairs);
  RG_CHECK(k >= 1 && k <= SEG_TOPK_MAX, "rg_segment_topk: k=%d not in 1..%d", k, SEG_TOPK_MAX);
  RG_CHECK(n_keys >= 0, "rg_segment_topk: n_keys=%lld", (long long)n_keys);
  RG_CHECK(n_keys == 0 || (q_key && known_keys && known_ptr && known_idx), "rg_segment_topk: n_keys=%lld with a NULL index array",
           (long long)n_keys);
  const hipStream_t s = (hipStream_t)stream;
  if (seg_ptr_is64)
    return launch(scores, ent, n_pairs, (const int64_t*)seg_ptr, batch, k, q_key, known_keys, known_ptr, known_idx, n_keys, idx_out,
                  score_out, prob_out, s);
  return launch(scores, ent, n_pairs, (const int32_t*)seg_ptr, batch, k, q_key, known_keys, known_ptr, known_idx, n_keys, idx_out,
                score_out, prob_out, s);
}
