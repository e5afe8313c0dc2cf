// Filtered top-k of a score matrix (include/redgnn.h: rg_topk): per row (s, r) the k best entities that are not already known tails of
// (s, r), ordered by score descending and entity id ascending.
//
// One workgroup per row.  Every entity j gets a unique 64-bit order key
//   K(j) = key32(score_j) << 32 | (0xFFFFFFFF - j)        (larger = better)
// with key32 order-preserving (NaN lowest, -0 == +0), so "k best" is "the k largest K" and ties by id need no separate rule.
// A radix select on K with 8-bit digits, most significant first, narrows the prefix of the k-th largest key: per pass a histogram in
// LDS over the entries that match the prefix so far, minus the known tails' entries (a loop over the row's known list, found by a
// 64-ary search of known_keys), then one wave picks the digit.  The select ends as soon as the chosen bin is taken whole (usually
// after 2-3 passes; rows with heavy ties go on into the id digits).  Then every entity whose K has a prefix >= the selected one is
// gathered into LDS (exactly min(k, #remaining) entries), sorted by a bitonic sort and written out.
//
// STAGED: the row's key32 values are kept in LDS after the first pass (rows up to TOPK_STAGE_MAX entities); otherwise each pass
// re-reads the row from global memory (L2 / MALL).  Only integer LDS atomics: the result does not depend on timing.
#include "select.h"

namespace {

constexpr int TT = 512;                 // threads per row
constexpr int TW = TT / 64;             // waves
constexpr int TOPK_MAX = 1024;
constexpr int32_t TOPK_STAGE_MAX = 32768;    // 128 KiB of key32 + 16 KiB of histograms and candidates <= 160 KiB

// layout of the dynamic LDS: [sub-histograms int32 TW x 256][candidates uint64 TOPK_MAX][control int32 16][key32 n_ent (STAGED)]
constexpr size_t LDS_HIST = (size_t)TW * 256 * 4, LDS_CAND = (size_t)TOPK_MAX * 8, LDS_CTRL = 16 * 4;
constexpr size_t LDS_FIXED = LDS_HIST + LDS_CAND + LDS_CTRL;

// key32 of the row's entries j0 + u*TT, u < UNR, all loads issued before any is used (UNR of them in flight per thread: a wide row is
// re-read from L2 / MALL on every pass, and one workgroup per row leaves most CUs with few waves to hide that latency); past the row: 0
constexpr int UNR = 8;
template <bool FROM_LDS>
__device__ __forceinline__ void row_keys(const float* __restrict__ grow, const uint32_t* s_key, uint32_t j0, uint32_t n,
                                         uint32_t (&kk)[UNR]) {
  float v[UNR];
#pragma unroll
  for (int u = 0; u < UNR; ++u) {
    const uint32_t j = j0 + u * TT;
    if (FROM_LDS) kk[u] = j < n ? s_key[j] : 0u;
    else v[u] = j < n ? grow[j] : 0.f;
  }
  if (!FROM_LDS) {
#pragma unroll
    for (int u = 0; u < UNR; ++u) kk[u] = key32(v[u]);
  }
}

// is j among known[lo, hi) (ascending)?
__device__ __forceinline__ bool known_has(const int32_t* __restrict__ known, int64_t lo, int64_t hi, int32_t j) {
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int32_t v = known[mid];
    if (v == j) return true;
    if (v < j) lo = mid + 1; else hi = mid;
  }
  return false;
}

template <bool STAGED>
__global__ __launch_bounds__(TT) void topk_kernel(const float* __restrict__ scores, int32_t n_ent, int32_t k,
                                                   const int64_t* __restrict__ q_key, const int64_t* __restrict__ known_keys,
                                                   const int64_t* __restrict__ known_ptr, const int32_t* __restrict__ known_idx,
                                                   int64_t n_keys, int32_t* __restrict__ idx_out, float* __restrict__ score_out) {
  extern __shared__ __align__(16) unsigned char lds[];
  int32_t* sub = reinterpret_cast<int32_t*>(lds);                                  // [TW][256]
  uint64_t* cand = reinterpret_cast<uint64_t*>(lds + LDS_HIST);                      // [TOPK_MAX]
  int32_t* ctrl = reinterpret_cast<int32_t*>(lds + LDS_HIST + LDS_CAND);            // [16]
  int64_t* ctrl64 = reinterpret_cast<int64_t*>(ctrl);                                // ctrl[0..3] = known range [kb, ke)
  uint32_t* s_key = reinterpret_cast<uint32_t*>(lds + LDS_FIXED);                    // [n_ent] (STAGED)

  const int64_t row = blockIdx.x;
  const float* __restrict__ grow = scores + row * (int64_t)n_ent;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int32_t* my_sub = sub + w * 256;

  for (int i = tid; i < TW * 256; i += TT) sub[i] = 0;
  // the row's known tails: 64-ary search of known_keys by wave 0 (a few dependent loads instead of ~log2(n_keys))
  if (w == 0) {
    int64_t kb = 0, ke = 0;
    if (n_keys > 0) {
      const int64_t q = q_key[row];
      int64_t lo = 0, hi = n_keys;                       // first index with known_keys[idx] >= q lies in [lo, hi]
      while (hi - lo >= 64) {
        const int64_t step = (hi - lo + 63) / 64;
        const int64_t p = lo + lane * step;
        const bool below = p < hi && known_keys[p] < q;
        const int c = __popcll(__ballot(below));         // lanes 0..c-1 are below q
        const int64_t nlo = c > 0 ? lo + (int64_t)(c - 1) * step + 1 : lo;
        const int64_t nhi = c < 64 ? min(hi, lo + (int64_t)c * step) : hi;
        lo = nlo; hi = nhi;
      }
      const int64_t p = lo + lane;
      const bool hit = p <= hi && p < n_keys && known_keys[p] == q;     // hi - lo <= 63: the lanes cover [lo, hi]
      const uint64_t m = __ballot(hit);
      if (m) {
        const int64_t at = lo + __ffsll((long long)m) - 1;
        kb = known_ptr[at];
        ke = known_ptr[at + 1];
      }
    }
    if (tid == 0) { ctrl64[0] = kb; ctrl64[1] = ke; }
  }
  __syncthreads();
  const int64_t kb = ctrl64[0], ke = ctrl64[1];

  int32_t need = k;
  uint64_t prefix = 0;
  int plen = 0;                    // bits of the selected prefix; 0 = every remaining entity is selected
  bool done = false;
  for (int d = 0; d < 8 && !done; ++d) {
    const int shift = 56 - 8 * d;
    // id digits that every id shares (ids < 2^s have 0xFF above bit s of 0xFFFFFFFF - j): nothing to count
    if (d >= 4 && ((uint32_t)(n_ent - 1) >> shift) == 0u) {
      prefix = (prefix << 8) | 0xFFu;
      plen += 8;
      continue;
    }
    const int hs = 64 - plen;      // prefix test: (K >> hs) == prefix (plen > 0)
    for (uint32_t j0 = tid; j0 < (uint32_t)n_ent; j0 += UNR * TT) {     // (j0 + UNR*TT < 2^32: n_ent < 2^31)
      uint32_t kk[UNR];
      if (STAGED && d > 0) row_keys<true>(grow, s_key, j0, (uint32_t)n_ent, kk);
      else row_keys<false>(grow, s_key, j0, (uint32_t)n_ent, kk);
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t j = j0 + u * TT;
        if (j >= (uint32_t)n_ent) break;
        if (STAGED && d == 0) s_key[j] = kk[u];
        const uint64_t K = order_key(kk[u], j);
        if (plen == 0 || (K >> hs) == prefix) atomicAdd(&my_sub[(K >> shift) & 0xFF], 1);
      }
    }
    __syncthreads();
    for (int64_t i = kb + tid; i < ke; i += TT) {          // the known tails do not count (each once, in range)
      const int32_t j = known_idx[i];
      if (j < 0 || j >= n_ent || (i > kb && known_idx[i - 1] == j)) continue;
      const uint64_t K = order_key(STAGED ? s_key[j] : key32(grow[j]), (uint32_t)j);
      if (plen == 0 || (K >> hs) == prefix) atomicSub(&my_sub[(K >> shift) & 0xFF], 1);
    }
    __syncthreads();
    if (w == 0) {
      // lane l holds bins 255-4l .. 252-4l (descending), reads and clears them; an inclusive scan over lanes finds the bin of the
      // need-th largest key
      int c[4], s = 0;
      for (int i = 0; i < 4; ++i) {
        const int b = 255 - 4 * lane - i;
        int t = 0;
        for (int v = 0; v < TW; ++v) { t += sub[v * 256 + b]; sub[v * 256 + b] = 0; }
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
        if (lane == 0) { ctrl[4] = 1; ctrl[5] = 0; ctrl[6] = total; ctrl[7] = 1; }   // fewer than k remain: take them all
      } else {
        const uint64_t m = __ballot(excl < need && need <= incl);
        const int at = m ? __ffsll((long long)m) - 1 : -1;
        if (at < 0) {
          if (lane == 0) { ctrl[4] = 1; ctrl[5] = 0; ctrl[6] = need; ctrl[7] = 1; }   // inconsistent counts (unsorted known list)
        } else if (lane == at) {
          int above = excl, i = 0;
          while (i < 3 && need > above + c[i]) { above += c[i]; ++i; }
          const int rem = need - above;
          ctrl[4] = 0; ctrl[5] = 255 - 4 * lane - i; ctrl[6] = rem; ctrl[7] = c[i] == rem;
        }
      }
    }
    __syncthreads();
    if (ctrl[4]) {                   // everything that remains
      need = ctrl[6];
      plen = 0;
      prefix = 0;
      done = true;
    } else {
      prefix = (prefix << 8) | (uint64_t)ctrl[5];
      plen += 8;
      need = ctrl[6];
      done = ctrl[7] != 0;
    }                                // (the next pass rewrites ctrl only after two more barriers)
  }

  // gather the selected keys (exactly `need` of them for a consistent known list; never more than TOPK_MAX are stored)
  if (tid == 0) ctrl[8] = 0;
  __syncthreads();
  const int hs = 64 - plen;
  for (uint32_t j0 = tid; j0 < (uint32_t)n_ent; j0 += UNR * TT) {
    uint32_t kk[UNR];
    row_keys<STAGED>(grow, s_key, j0, (uint32_t)n_ent, kk);
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const uint32_t j = j0 + u * TT;
      if (j >= (uint32_t)n_ent) break;
      const uint64_t K = order_key(kk[u], j);
      if ((plen == 0 || (K >> hs) >= prefix) && !known_has(known_idx, kb, ke, (int32_t)j)) {
        const int pos = atomicAdd(&ctrl[8], 1);
        if (pos < TOPK_MAX) cand[pos] = K;
      }
    }
  }
  __syncthreads();
  const int n = min(min(ctrl[8], k), TOPK_MAX);
  int P = 1;
  while (P < n) P <<= 1;
  for (int i = n + tid; i < P; i += TT) cand[i] = 0;      // below every real key (its id word is >= 2^31)
  __syncthreads();
  // bitonic sort, descending
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += TT) {
        const int i = 2 * t - (t & (stride - 1));
        const int jx = i + stride;
        const bool desc = (i & size) == 0;
        const uint64_t a = cand[i], b = cand[jx];
        if ((a < b) == desc) { cand[i] = b; cand[jx] = a; }
      }
      __syncthreads();
    }
  }
  int32_t* irow = idx_out + row * (int64_t)k;
  float* srow = score_out + row * (int64_t)k;
  for (int i = tid; i < k; i += TT) {
    if (i < n) {
      const uint32_t j = 0xFFFFFFFFu - (uint32_t)cand[i];
      irow[i] = (int32_t)j;
      srow[i] = grow[j];
    } else {
      irow[i] = -1;
      srow[i] = -INFINITY;
    }
  }
}

}  // namespace

extern "C" int rg_topk(const float* scores, int32_t batch, int32_t n_ent, int32_t k, const int64_t* q_key, const int64_t* known_keys,
                       const int64_t* known_ptr, const int32_t* known_idx, int64_t n_keys, int32_t* idx_out, float* score_out,
                       void* stream) {
  RG_CHECK(scores && idx_out && score_out, "rg_topk: NULL argument");
  RG_CHECK(batch > 0 && n_ent > 0, "rg_topk: batch=%d n_ent=%d", batch, n_ent);
  RG_CHECK(k >= 1 && k <= TOPK_MAX, "rg_topk: k=%d not in 1..%d", k, TOPK_MAX);
  RG_CHECK(n_keys >= 0, "rg_topk: n_keys=%lld", (long long)n_keys);
  RG_CHECK(n_keys == 0 || (q_key && known_keys && known_ptr && known_idx), "rg_topk: n_keys=%lld with a NULL index array",
           (long long)n_keys);
  const hipStream_t s = (hipStream_t)stream;
  if (n_ent <= TOPK_STAGE_MAX) {
    const size_t lds = LDS_FIXED + (size_t)n_ent * 4;
    if (lds > 64 * 1024) RG_HIP(hipFuncSetAttribute((const void*)topk_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(topk_kernel<true>, dim3(batch), dim3(TT), lds, s, scores, n_ent, k, q_key, known_keys, known_ptr, known_idx,
                       n_keys, idx_out, score_out);
  } else {
    hipLaunchKernelGGL(topk_kernel<false>, dim3(batch), dim3(TT), LDS_FIXED, s, scores, n_ent, k, q_key, known_keys, known_ptr,
                       known_idx, n_keys, idx_out, score_out);
  }
  RG_LAUNCH_CHECK();
  return 0;
}
