// The k best length-L paths s -> o of every row of a compact r-digraph (include/redgnn.h: rg_paths_topk), by alpha product.
//
// Input is the edge list as explain.RDigraph holds it: edges int32 [E, 5] = (row, hop, head, rel, tail) ordered by (row, hop, tail,
// CSR position), alpha fp32 [E], offsets int64 [B + 1].  No graph, frontier or model: a row's digraph is self-contained.
//
// Order.  A path's product is ((1.0 * a_1) * a_2) ... * a_L in float64.  P comes before Q at level l when P's product is larger;
// else when P's last edge has the smaller (head, rel, edge index); else, the last edge being the same, when P's prefix comes before
// Q's at level l - 1.  Rounding is monotone, so the k best paths into a node continue only the k best prefixes of their heads.
//
// One workgroup per row walks the hops with a barrier in between.  A "group" is a run of edges of one (row, hop, tail); its table
// entry - k slots of (product, last edge, rank of the prefix in the head's entry) and a count - sits at the group's first edge,
// so a hop-l edge finds its head's entry by a lower-bound search on `tail` inside the row's hop-(l-1) range.  Per hop:
//   1. the group starts are listed by a head flag and a block scan over 256-edge tiles;
//   2. one wave per group: every lane keeps the k best of its strided candidates (edge x prefix slot) in registers, sorted, and k
//      rounds of a wave-wide arg-max take the group's list from the lanes' list heads.
// The row's answer is the entry of the group of its last edge (explain gives hop L the single tail o); k threads walk it back.
//
// Every index derived from the edge list is bounded by the row's [offsets[b], offsets[b + 1]); the counts are cleared before the
// first hop, so an entry that a malformed (unsorted) list reaches without it being a group start is empty, never stale.
#include <hipcub/hipcub.hpp>

#include "common.h"

namespace {

constexpr int PT = 256;                 // threads per row
constexpr int PW = PT / 64;             // waves
constexpr int PATHS_MAX_K = 8;
constexpr int PATHS_MAX_HOPS = 32;
constexpr size_t PATHS_ALIGN = 256;

// slices of the scratch for n edges: product double [n, k], last edge int32 [n, k] (row-local), list of group starts int32 [n],
// prefix rank uint8 [n, k], count uint8 [n]
struct Tables {
  double* prod;
  int32_t* back;
  int32_t* glist;
  uint8_t* rank;
  uint8_t* cnt;
};

__host__ __device__ inline size_t up(size_t x) { return (x + PATHS_ALIGN - 1) / PATHS_ALIGN * PATHS_ALIGN; }

__host__ __device__ inline size_t carve(void* scratch, int64_t n, int k, Tables* t) {
  unsigned char* p = static_cast<unsigned char*>(scratch);
  size_t o = 0;
  if (t) t->prod = reinterpret_cast<double*>(p + o);
  o += up((size_t)n * k * 8);
  if (t) t->back = reinterpret_cast<int32_t*>(p + o);
  o += up((size_t)n * k * 4);
  if (t) t->glist = reinterpret_cast<int32_t*>(p + o);
  o += up((size_t)n * 4);
  if (t) t->rank = reinterpret_cast<uint8_t*>(p + o);
  o += up((size_t)n * k);
  if (t) t->cnt = reinterpret_cast<uint8_t*>(p + o);
  o += up((size_t)n);
  return o + PATHS_ALIGN;
}

// A candidate path into a group: its product, (head << 32 | rel) of its last edge, (last edge << 3 | prefix rank).  All-ones keys
// with product -inf: no candidate.
struct Cand {
  double p;
  uint64_t hr, ej;
};

__device__ __forceinline__ Cand none() { return Cand{-INFINITY, ~0ull, ~0ull}; }

__device__ __forceinline__ bool before(const Cand& a, const Cand& b) {
  if (a.p > b.p) return true;
  if (a.p < b.p) return false;
  if (a.hr != b.hr) return a.hr < b.hr;
  return a.ej < b.ej;
}

// first i in [lo, hi) with col[5 * i] >= x (the column ascending there; any content gives an index in [lo, hi])
__device__ __forceinline__ int32_t lower_bound5(const int32_t* __restrict__ col, int32_t lo, int32_t hi, int32_t x) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (col[5 * (int64_t)mid] < x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ double wave_max(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t y = __shfl_xor((unsigned long long)v, o, 64);
    v = y < v ? y : v;
  }
  return v;
}

template <int K>
__global__ __launch_bounds__(PT) void paths_topk_kernel(const int32_t* __restrict__ edges, const float* __restrict__ alpha,
                                                        const int64_t* __restrict__ offsets, int32_t row_lo, int32_t row_hi,
                                                        int32_t n_hops, void* scratch, int64_t* __restrict__ path_edge,
                                                        double* __restrict__ path_prod, int32_t* __restrict__ path_count) {
  using Scan = hipcub::BlockScan<int32_t, PT>;
  __shared__ typename Scan::TempStorage s_scan;
  __shared__ int32_t s_hop[PATHS_MAX_HOPS + 2];       // s_hop[l] = first edge of hop l in the row (row-local), s_hop[L + 1] = their end

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t row = (int64_t)row_lo + blockIdx.x;
  const int L = n_hops;
  // the row's edges, clamped into the chunk's range (what the scratch was sized for)
  const int64_t base = offsets[row_lo], lim = max(offsets[row_hi], base);
  const int64_t e0 = min(max(offsets[row], base), lim), e1 = min(max(offsets[row + 1], e0), lim);
  const int32_t n = (int32_t)(e1 - e0);
  const int32_t* __restrict__ E = edges + 5 * e0;       // row-local edge i: E[5 * i + {0: row, 1: hop, 2: head, 3: rel, 4: tail}]
  const float* __restrict__ A = alpha + e0;
  Tables t;
  carve(scratch, lim - base, K, &t);
  double* t_prod = t.prod + (e0 - base) * K;
  int32_t* t_back = t.back + (e0 - base) * K;
  uint8_t* t_rank = t.rank + (e0 - base) * K;
  uint8_t* t_cnt = t.cnt + (e0 - base);
  int32_t* glist = t.glist + (e0 - base);

  for (int32_t i = tid; i < n; i += PT) t_cnt[i] = 0;
  if (tid >= 1 && tid <= L + 1) s_hop[tid] = lower_bound5(E + 1, 0, n, tid);
  __syncthreads();
  if (tid == 0) {                                       // ascending whatever the hop column holds
    s_hop[0] = 0;
    for (int l = 1; l <= L + 1; ++l) s_hop[l] = max(s_hop[l], s_hop[l - 1]);
  }
  __syncthreads();

  int32_t n_groups = 0;
  for (int l = 1; l <= L; ++l) {
    const int32_t a = s_hop[l], b = s_hop[l + 1], pa = s_hop[l - 1];      // this hop's edges [a, b), the hop before's [pa, a)
    // 1. group starts of the hop, in order, into glist[a ...]
    n_groups = 0;
    for (int32_t i0 = a; i0 < b; i0 += PT) {
      const int32_t i = i0 + tid;
      const int32_t flag = i < b && (i == a || E[5 * (int64_t)i + 4] != E[5 * (int64_t)(i - 1) + 4]);
      int32_t pos, total;
      Scan(s_scan).ExclusiveSum(flag, pos, total);
      if (flag) glist[a + n_groups + pos] = i;
      n_groups += total;
      __syncthreads();                                  // s_scan is reused by the next tile
    }
    // 2. one wave per group
    for (int32_t g = w; g < n_groups; g += PW) {
      const int32_t gs = glist[a + g], ge = g + 1 < n_groups ? glist[a + g + 1] : b;
      Cand best[K];
#pragma unroll
      for (int i = 0; i < K; ++i) best[i] = none();
      for (int32_t e = gs + lane; e < ge; e += 64) {
        const int32_t h = E[5 * (int64_t)e + 2], r = E[5 * (int64_t)e + 3];
        const double al = (double)A[e];
        const uint64_t hr = (uint64_t)(uint32_t)h << 32 | (uint32_t)r;
        int32_t p = 0, np = 1;                          // the head's entry and its number of prefixes (hop 1: the empty prefix)
        if (l > 1) {
          p = lower_bound5(E + 4, pa, a, h);
          np = p < a && E[5 * (int64_t)p + 4] == h ? min((int)t_cnt[p], K) : 0;
        }
        for (int j = 0; j < np; ++j) {
          Cand c{(l > 1 ? t_prod[(int64_t)p * K + j] : 1.0) * al, hr, (uint64_t)(uint32_t)e << 3 | (uint32_t)j};
#pragma unroll
          for (int i = 0; i < K; ++i) {                 // sorted insertion, the loser carried down
            if (before(c, best[i])) { const Cand x = best[i]; best[i] = c; c = x; }
          }
        }
      }
      // K rounds: the best list head of the wave wins, its lane writes the slot and moves its list up
      int found = 0;
      for (int round = 0; round < K; ++round) {
        const Cand c = best[0];
        const bool valid = c.ej != ~0ull;
        const double m = wave_max(valid ? c.p : -INFINITY);
        uint64_t mask = __ballot(valid && c.p == m);
        if (__popcll(mask) > 1) {
          const bool in = (mask >> lane) & 1;
          const uint64_t hm = wave_min(in ? c.hr : ~0ull);
          mask = __ballot(in && c.hr == hm);
          if (__popcll(mask) > 1) {
            const bool in2 = (mask >> lane) & 1;
            const uint64_t em = wave_min(in2 ? c.ej : ~0ull);
            mask = __ballot(in2 && c.ej == em);
          }
        }
        if (mask == 0) break;                           // no candidate left (or only NaN products)
        if (lane == __ffsll((long long)mask) - 1) {
          t_prod[(int64_t)gs * K + round] = c.p;
          t_back[(int64_t)gs * K + round] = (int32_t)(c.ej >> 3);
          t_rank[(int64_t)gs * K + round] = (uint8_t)(c.ej & 7);
#pragma unroll
          for (int i = 0; i + 1 < K; ++i) best[i] = best[i + 1];
          best[K - 1] = none();
        }
        ++found;
      }
      if (lane == 0) t_cnt[gs] = (uint8_t)found;
    }
    __syncthreads();                                    // the hop's entries are complete (and glist may be rewritten)
  }

  // the answer: the entry of the last group of hop L, if the row's last edge is a hop-L edge
  const bool has = n > 0 && s_hop[L + 1] == n && s_hop[L] < n && n_groups > 0;
  const int32_t gl = has ? glist[s_hop[L] + n_groups - 1] : 0;
  const int count = has ? min((int)t_cnt[gl], K) : 0;
  if (tid == 0) path_count[row] = count;
  if (tid < K) {
    int64_t* pe = path_edge + (row * K + tid) * L;
    if (tid < count) {
      path_prod[row * K + tid] = t_prod[(int64_t)gl * K + tid];
      int32_t p = gl, j = tid;
      for (int l = L; l >= 1; --l) {
        const int32_t e = t_back[(int64_t)p * K + j];
        j = t_rank[(int64_t)p * K + j];
        pe[l - 1] = e0 + e;
        // the head's entry, found as the forward pass found it (s_hop[l - 1] < s_hop[l] there: the entry had a prefix)
        if (l > 1) p = min(lower_bound5(E + 4, s_hop[l - 1], s_hop[l], E[5 * (int64_t)e + 2]), max(s_hop[l] - 1, 0));
      }
    } else {
      path_prod[row * K + tid] = 0.0;
      for (int l = 0; l < L; ++l) pe[l] = -1;
    }
  }
}

template <int K>
int launch(const int32_t* edges, const float* alpha, const int64_t* offsets, int32_t row_lo, int32_t row_hi, int32_t n_hops,
           void* scratch, int64_t* path_edge, double* path_prod, int32_t* path_count, hipStream_t s) {
  hipLaunchKernelGGL(paths_topk_kernel<K>, dim3(row_hi - row_lo), dim3(PT), 0, s, edges, alpha, offsets, row_lo, row_hi, n_hops,
                     scratch, path_edge, path_prod, path_count);
  RG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" size_t rg_paths_scratch_bytes(int64_t n_edges, int32_t k) {
  if (n_edges < 0 || n_edges >= ((int64_t)1 << 31) || k < 1 || k > PATHS_MAX_K) return 0;
  return carve(nullptr, n_edges, k, nullptr);
}

extern "C" int rg_paths_topk(const int32_t* edges, const float* alpha, const int64_t* offsets, int32_t row_lo, int32_t row_hi,
                             int32_t n_hops, int32_t k, void* scratch, int64_t* path_edge, double* path_prod, int32_t* path_count,
                             void* stream) {
  RG_CHECK(offsets && scratch && path_edge && path_prod && path_count, "rg_paths_topk: NULL argument");
  RG_CHECK(row_lo >= 0 && row_hi >= row_lo, "rg_paths_topk: rows %d..%d", row_lo, row_hi);
  RG_CHECK(n_hops >= 1 && n_hops <= PATHS_MAX_HOPS, "rg_paths_topk: n_hops=%d not in 1..%d", n_hops, PATHS_MAX_HOPS);
  RG_CHECK(k >= 1 && k <= PATHS_MAX_K, "rg_paths_topk: k=%d not in 1..%d", k, PATHS_MAX_K);
  if (row_hi == row_lo) return 0;
  RG_CHECK(edges && alpha, "rg_paths_topk: NULL edge list");
  const hipStream_t s = (hipStream_t)stream;
#define RG_PATHS_K(K_) \
  case K_: return launch<K_>(edges, alpha, offsets, row_lo, row_hi, n_hops, scratch, path_edge, path_prod, path_count, s);
  switch (k) {
    RG_PATHS_K(1) RG_PATHS_K(2) RG_PATHS_K(3) RG_PATHS_K(4) RG_PATHS_K(5) RG_PATHS_K(6) RG_PATHS_K(7) RG_PATHS_K(8)
  }
#undef RG_PATHS_K
  return 1;
}
