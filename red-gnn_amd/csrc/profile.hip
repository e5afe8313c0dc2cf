// Attention profile of a hop: per query b and edge relation rel, the number of hop-l edges of b's subgraph with that relation and
// the sum of their attention alpha (the reference's attention_vis table, Temporal/interpolation/model_cuda.py:117-119,163-166,
// without its python loop over relations and its two .item() read-backs per relation and layer).
//
// The edges are the ones the forward aggregates: the in-edges (h, rel, t) of every tail t in level l of query b whose head h is in
// level l-1 of the same query (identity edges included, duplicated facts counted once each).  Level l IS the set of tails of the
// out-edges of level l-1 (rg_frontier_expand), so the same edges are all out-edges of the level-(l-1) nodes, and that is how they are
// enumerated here: from the heads through the CSR by head.  Unlike the walk by tail (explain.hip, which has to start from marked
// tails) no candidate edge is read in vain - on a first hop the tails' in-edges outnumber the hop's edges by two orders of magnitude
// - no bitmap word is looked up per edge, and the a_s row is one per head, shared by the lanes on its out-edges.  alpha is the forward
// kernel's arithmetic (the same attn.h calls in the forward's operand order), so it is the forward's alpha bit for bit; sums of
// integers do not depend on the order of enumeration.
//
// Work mapping: blockIdx.y = query, so a workgroup's bins belong to one query.  A wave takes `gw` consecutive words of the
// query's level-(l-1) bitmap at a time (one word per lane), lists their set bits (the heads) in LDS, and then flattens the heads'
// CSR rows 64 heads at a time: a wave scan of the out-degrees, and for every 64 consecutive positions of the concatenated rows a
// binary search of that scan (shuffles) gives each lane its head.  Every lane then holds one edge whatever the degrees are,
// and lanes on the same head read consecutive CSR entries and the same a_s row.  Per edge: 8 B of CSR, a_r from LDS; per head
// an ap-wide a_s row; no state row.
//
// Sums are order-free and exact: alpha is added as 64-bit fixed point, llrintf(alpha * 2^32) (alpha in [0, 1]; 2^31 edges stay
// below 2^63), so the per-edge rounding is q = 2^-33 and integer addition makes the result independent of scheduling, of how a
// batch is cut and of the order of its queries.  The relation bins (sum 8 B + count 4 B, beside the a_r table) are private to the
// workgroup in LDS and flushed once with non-returning 64-bit integer atomics into the caller's [B][n_rela_rows] buffers.  Where the
// table and the bins do not fit 48 KB of LDS (n_rela_rows * (4 * ap + 12) bytes: thousands of relations) the same kernel adds per
// edge into the global buffers with the same integer atomics and reads a_r from memory: slower, same result.
//
// Temporal graphs (rg_tattn_profile, T-RED-GNN interpolation): the kernel's DIR instantiation.  The enumeration is the same; per
// edge it also reads out_time[entry] (4 B more of CSR) and bins by the forward's direction (tlayer_fwd.hip): dt = edge time -
// q_time[b], dir 0 past (dt < 0), 1 now (dt == 0), 2 future (dt > 0); bin = dir * n_rela_rows + rel, outputs [B][3][n_rela_rows].  The
// temporal attention does not read the time, so alpha is the static arithmetic.  Three bins per relation: the LDS path needs
// n_rela_rows * (4 * ap + 36) bytes beside the 16 KB head list in 64 KB, i.e. at most 49152 / (4 * ap + 36) relation rows (945 at
// ap = 4, 722 at ap = 8, 491 at ap = 16, 299 at ap = 32); above that the global-atomic path runs (same integers).
//
// Extrapolation (rg_xattn_profile, extrapolation.py's one-graph layout): the kernel's LAG instantiation.  out_time[entry] is the edge's
// data row and the frontier carries the queries' row windows.  An out-edge of a level-(l-1) node of query b is a hop-l edge of b iff its
// row is a self-loop (row >= n_data) or lies in [win_lo[b], win_hi[b]) - the forward's test (layer_fwd_kernel.h), n_data and the windows
// taken from the frontier as rg_xexplain_* takes them.  Enumeration from the heads stays valid under a window: the windowed
// rg_frontier_expand (hop_or_window_kernel) makes level l precisely the set of tails of these edges, so every edge that passes the
// test ends in level l and no tail bitmap is read.  A head's CSR row is read over all times and filtered per edge, as the forward
// does it.  The time does not enter alpha.  The edge is binned by the forward's time-table row:
//   lag = min(max(q_time[b] - (row >= n_data ? loop_time[b] : row_time[row]), 0), n_lag - 1),  bin = lag_bin[lag]
// with lag_bin a device uint8 [n_lag] table staged in LDS on both paths; cell = bin * n_rela_rows + rel, outputs
// [B][n_bins][n_rela_rows].  An entry >= n_bins drops the edge, so no table content can make the kernel write outside the outputs.
// 1 <= n_bins <= 256, 1 <= n_lag <= 16384.
// LDS budget of this mode: 80 KiB per workgroup (two workgroups per CU of 160 KiB; hipFuncAttributeMaxDynamicSharedMemorySize is
// raised above 64 KB), and the LDS path runs where
//   16384 (head list) + n_rela_rows * (4 * ap + 12 * n_bins) + n_lag <= 81920
// - ICEWS14's 462 relation rows at ap = 8 with 8 bins need 75.9 KB.  Which budget is faster has NOT been measured: 160 KiB would keep
// larger tables in LDS at one workgroup (four waves) per CU, 64 KB would keep three workgroups per CU and send ICEWS14 to the
// global-atomic path.  Above the budget the global-atomic path runs with the head list and the lag table in LDS (same integers).
#include <algorithm>

#include "attn.h"

namespace {

constexpr int PF_BLOCK = 256;
constexpr int PF_WAVES = PF_BLOCK / 64;
constexpr int PF_HEADS = 64 * 32;                      // heads of one wave step (64 words)
constexpr size_t PF_LIST_BYTES = (size_t)PF_WAVES * PF_HEADS * sizeof(uint16_t);
constexpr size_t PF_LDS_MAX = 64 * 1024;
constexpr float PF_SCALE = 4294967296.0f;              // 2^32

struct PfArgs {
  const int2* bm_old;        // level l-1 {word, prefix} [B][W]
  int W, n_ent, n_old;
  int gw, n_groups;          // words per wave step (power of two <= 64), ceil(W / gw)
  const int32_t* out_ptr;    // CSR by head
  const int2* out_rt;        // {rel, tail}
  const float4* a_s;         // [N_{l-1}][AP4]
  const float4* a_r;         // [R][AP4]
  const float4* a_q;         // [B][AP4]
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  int R;                     // n_rela_rows
  unsigned long long* sum_out;     // [B][R]
  unsigned long long* count_out;   // [B][R]
};

__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

struct TPfArgs : PfArgs {
  const int32_t* out_time;   // time id of every CSR-by-head entry
  const int32_t* q_time;     // [B]
};

struct XPfArgs : PfArgs {
  const int32_t* out_time;   // data row of every CSR-by-head entry (>= n_data: a self-loop)
  const int32_t* q_time;     // [B]
  const int32_t* loop_time;  // [B] the day the forward gives query b's self-loops
  const int32_t* row_time;   // [n_data] day of every data row
  const int32_t* win_lo;     // [B] first data row of the query's window
  const int32_t* win_hi;     // [B] one past its last
  const uint8_t* lag_bin;    // [n_lag]
  int n_data, n_lag, n_lbins;
};

constexpr int XPF_N_LAG_MAX = 16384;                   // the lag table is staged in LDS on both paths
#ifndef RG_XPF_LDS_KIB
#define RG_XPF_LDS_KIB 80                              // the LAG mode's budget (two workgroups per CU); -DRG_XPF_LDS_KIB=64..160 builds an A/B variant
#endif
constexpr size_t XPF_LDS_MAX = (size_t)RG_XPF_LDS_KIB * 1024;
static_assert(RG_XPF_LDS_KIB >= 64 && RG_XPF_LDS_KIB <= 160, "the LAG budget: 64..160 KiB");

template <bool DIR, bool LAG>
using PfArgsOf = std::conditional_t<LAG, XPfArgs, std::conditional_t<DIR, TPfArgs, PfArgs>>;

template <int AP4, bool LDS, bool DIR = false, bool LAG = false>
__global__ __launch_bounds__(PF_BLOCK) void profile_kernel(PfArgsOf<DIR, LAG> A) {
  extern __shared__ __align__(16) unsigned char pf_smem[];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int b = blockIdx.y;
  uint16_t* heads = (uint16_t*)pf_smem + wv * PF_HEADS;
  float4* ar_l = (float4*)(pf_smem + PF_LIST_BYTES);
  int n_bins = DIR ? 3 * A.R : A.R;                     // (direction | lag bin, relation) cells of one query
  if constexpr (LAG) n_bins = A.n_lbins * A.R;
  unsigned long long* sum_l = (unsigned long long*)(ar_l + (LDS ? A.R * AP4 : 0));
  uint32_t* cnt_l = (uint32_t*)(sum_l + (LDS ? n_bins : 0));
  if constexpr (LDS) {
    for (int i = threadIdx.x; i < A.R * AP4; i += PF_BLOCK) ar_l[i] = A.a_r[i];
    for (int i = threadIdx.x; i < n_bins; i += PF_BLOCK) { sum_l[i] = 0ull; cnt_l[i] = 0u; }
    __syncthreads();
  }
  int qt = 0;
  if constexpr (DIR) qt = A.q_time[b];
  int wlo = 0, whi = 0, loop_t = 0;
  uint8_t* lag_l = (uint8_t*)(cnt_l + (LDS ? n_bins : 0));
  if constexpr (LAG) {
    qt = A.q_time[b]; loop_t = A.loop_time[b]; wlo = A.win_lo[b]; whi = A.win_hi[b];
    for (int i = threadIdx.x; i < A.n_lag; i += PF_BLOCK) lag_l[i] = A.lag_bin[i];
    __syncthreads();
  }
  const float b_alpha = A.b_alpha[0];
  float4 w[AP4], q[AP4];
#pragma unroll
  for (int k = 0; k < AP4; ++k) {
    w[k] = rg::attn_w4(A.w_alpha, A.attn_dim, k);
    q[k] = A.a_q[(int64_t)b * AP4 + k];
  }
  const int2* bm_old = A.bm_old + (int64_t)b * A.W;
  unsigned long long* sum_g = A.sum_out + (int64_t)b * n_bins;
  unsigned long long* cnt_g = A.count_out + (int64_t)b * n_bins;

  for (int g = blockIdx.x * PF_WAVES + wv; g < A.n_groups; g += gridDim.x * PF_WAVES) {   // (uniform over the wave)
    // ---- the heads of this step: set bits of gw words, listed in LDS in entity order, with their node ids ----------------
    const int wl = g * A.gw + lane;
    const int2 wp = (lane < A.gw && wl < A.W) ? bm_old[wl] : make_int2(0, 0);
    uint32_t bits = (uint32_t)wp.x;
    if (wl == A.W - 1 && (A.n_ent & 31)) bits &= (1u << (A.n_ent & 31)) - 1u;   // never an entity past n_ent
    const int nb = __popc(bits);
    const int incl_b = wave_incl_scan(nb, lane);
    const int n_heads = __shfl(incl_b, 63, 64);
    const int off = incl_b - nb;
    for (int i = 0; bits; ++i) {
      heads[off + i] = (uint16_t)(lane * 32 + __ffs((int)bits) - 1);
      bits &= bits - 1u;
    }
    // node id of the step's k-th head: the first word's prefix + k (the prefix runs over the query's words in order)
    const int s_base = __shfl(wp.y, 0, 64);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int e_base = g * A.gw * 32;
    for (int k0 = 0; k0 < n_heads; k0 += 64) {
      // ---- 64 heads, one per lane: their CSR rows laid end to end --------------------------------------------------------
      int beg = 0, deg = 0;
      if (k0 + lane < n_heads) {
        const int h = e_base + heads[k0 + lane];
        beg = A.out_ptr[h];
        deg = A.out_ptr[h + 1] - beg;
      }
      const int incl_d = wave_incl_scan(deg, lane);
      const int excl_d = incl_d - deg;
      const int total = __shfl(incl_d, 63, 64);
      for (int x0 = 0; x0 < total; x0 += 64) {
        const int x = x0 + lane;
        int sl = 0;                                   // the head of position x: the first lane whose inclusive scan exceeds x
#pragma unroll
        for (int step = 32; step > 0; step >>= 1) {
          const int v = __shfl(incl_d, sl + step - 1, 64);
          if (v <= x) sl += step;
        }
        const int beg_s = __shfl(beg, sl, 64), excl_s = __shfl(excl_d, sl, 64);
        if (x < total) {
          const int entry = beg_s + (x - excl_s);
          const int r = A.out_rt[entry].x;
          const int s = s_base + k0 + sl;
          bool keep = (uint32_t)r < (uint32_t)A.R && s < A.n_old;
          int bin = r;
          if constexpr (LAG) {
            if (keep) {                               // the forward's window test and time-table row (layer_fwd_kernel.h)
              const int row = A.out_time[entry];
              keep = row >= A.n_data || (row >= wlo && row < whi);
              if (keep) {
                const int lag = min(max(qt - (row >= A.n_data ? loop_t : A.row_time[row]), 0), A.n_lag - 1);
                const int lb = lag_l[lag];
                keep = lb < A.n_lbins;                // an entry outside the bins drops the edge: never a cell past the outputs
                bin = lb * A.R + r;
              }
            }
          }
          if (keep) {
            float z = b_alpha;
#pragma unroll
            for (int k = 0; k < AP4; ++k) {
              const float4 as = A.a_s[(int64_t)s * AP4 + k];
              float4 ar;
              if constexpr (LDS) ar = ar_l[r * AP4 + k]; else ar = A.a_r[(int64_t)r * AP4 + k];
              rg::attn_acc_fwd(z, w[k], as, ar, q[k]);
            }
            const float alpha = rg::attn_alpha(z);
            const unsigned long long fx = (unsigned long long)llrintf(alpha * PF_SCALE);
            if constexpr (DIR) {
              const int dt = A.out_time[entry] - qt;
              bin = (dt > 0 ? 2 : (dt == 0 ? 1 : 0)) * A.R + r;
            }
            // results unused: non-returning integer adds, order-free
            if constexpr (LDS) {
              atomicAdd(&sum_l[bin], fx);
              atomicAdd(&cnt_l[bin], 1u);
            } else {
              atomicAdd(&sum_g[bin], fx);
              atomicAdd(&cnt_g[bin], 1ull);
            }
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the list is read out before the next step overwrites it
    __builtin_amdgcn_wave_barrier();
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_bins; i += PF_BLOCK) {
      const uint32_t c = cnt_l[i];
      if (c) {
        atomicAdd(&sum_g[i], sum_l[i]);
        atomicAdd(&cnt_g[i], (unsigned long long)c);
      }
    }
  }
}

// the lag arguments of rg_xattn_profile
struct LagTable {
  const int32_t* loop_time;
  const int32_t* row_time;
  const uint8_t* lag_bin;
  int32_t n_lag, n_bins;
};

// the entry points' checks and launch; DIR = the temporal profile (q_time non-NULL), LAG = the extrapolation profile (q_time and x)
template <bool DIR, bool LAG = false>
int profile_hop(const char* who, const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                const int32_t* q_time, const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                const float* b_alpha, int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream, const LagTable* x = nullptr) {
  RG_CHECK(level >= 1 && level < RG_MAX_LEVELS, "%s: level %d not in 1..%d", who, level, RG_MAX_LEVELS - 1);
  RG_CHECK(batch > 0 && n_ent > 0, "%s: batch=%d n_ent=%d must be positive", who, batch, n_ent);
  RG_CHECK(a_s && a_r && a_q && w_alpha && b_alpha && sum_out && count_out && (!(DIR || LAG) || q_time), "%s: NULL argument", who);
  if constexpr (LAG) {
    RG_CHECK(x->loop_time && x->row_time && x->lag_bin, "%s: NULL argument", who);
    RG_CHECK(x->n_bins >= 1 && x->n_bins <= 256, "%s: n_bins=%d not in 1..256", who, x->n_bins);
    RG_CHECK(x->n_lag >= 1 && x->n_lag <= XPF_N_LAG_MAX, "%s: n_lag=%d not in 1..%d", who, x->n_lag, XPF_N_LAG_MAX);
  }
  RG_CHECK(attn_dim > 0 && ap >= attn_dim && ap % 4 == 0 && ap <= 32, "%s: attn_dim=%d ap=%d (attention widths up to 32, ap a multiple of 4)",
           who, attn_dim, ap);
  RG_CHECK((((uintptr_t)a_s | (uintptr_t)a_r | (uintptr_t)a_q) & 15) == 0, "%s: attention tables must be 16-B aligned", who);
  RG_CHECK((((uintptr_t)sum_out | (uintptr_t)count_out) & 7) == 0, "%s: output buffers must be 8-B aligned", who);
  RG_CHECK(f != nullptr && g != nullptr, "%s: NULL frontier or graph", who);
  RG_CHECK(batch == f->B && n_ent == f->n_ent, "%s: batch=%d n_ent=%d but the frontier has batch %d, n_ent %d", who, batch, n_ent,
           f->B, f->n_ent);
  RG_CHECK(g->n_ent == f->n_ent, "%s: graph has %d entities, frontier %d", who, g->n_ent, f->n_ent);
  if constexpr (LAG) {
    RG_CHECK(g->n_time > 0 && g->out_time, "%s: the graph has no row ids (build it with rg_tgraph_create, time field = data row)", who);
    RG_CHECK(f->win_lo && f->win_hi, "%s: the frontier has no window set (call rg_frontier_set_window first)", who);
  } else if constexpr (DIR) {
    RG_CHECK(g->n_time > 0 && g->out_time, "%s: temporal graphs only (rg_tgraph_create)", who);
    RG_CHECK(f->win_lo == nullptr, "%s: the frontier has a window set (extrapolation is not supported)", who);
  } else {
    RG_CHECK(g->n_time == 0 && f->win_lo == nullptr, "%s: static graphs only (rg_graph_create)", who);
  }
  RG_CHECK(level <= f->level && level > f->level - f->n_levels + 1, "%s: level %d not resident (current %d, %d kept)", who, level,
           f->level, f->n_levels);
  RG_CHECK(batch <= 65535, "%s: batch=%d above 65535 queries per call", who, batch);
  const int64_t n_have = f->n_nodes[(level - 1) % f->n_levels];
  RG_CHECK(n_have >= 0 && n_old == n_have, "%s: n_old=%lld but level %d has %lld nodes", who, (long long)n_old, level - 1, (long long)n_have);
  PfArgsOf<DIR, LAG> A;
  RG_CHECK(n_old <= INT32_MAX, "%s: n_old=%lld does not fit int32", who, (long long)n_old);
  A.bm_old = f->bm_of(level - 1); A.W = f->W; A.n_ent = f->n_ent; A.n_old = (int)n_old;
  A.out_ptr = g->out_ptr; A.out_rt = g->out_rt;
  A.a_s = (const float4*)a_s; A.a_r = (const float4*)a_r; A.a_q = (const float4*)a_q;
  A.w_alpha = w_alpha; A.b_alpha = b_alpha; A.attn_dim = attn_dim; A.R = g->n_rela_rows;
  A.sum_out = (unsigned long long*)sum_out; A.count_out = (unsigned long long*)count_out;
  if constexpr (DIR || LAG) { A.out_time = g->out_time; A.q_time = q_time; }
  if constexpr (LAG) {
    RG_CHECK((int64_t)x->n_bins * A.R <= INT32_MAX, "%s: n_bins=%d x %d relation rows does not fit int32", who, x->n_bins, A.R);
    A.loop_time = x->loop_time; A.row_time = x->row_time; A.lag_bin = x->lag_bin; A.n_lag = x->n_lag; A.n_lbins = x->n_bins;
    A.win_lo = f->win_lo; A.win_hi = f->win_hi; A.n_data = f->win_n_data;
  }
  // words per wave step: 64, less for small batches so that the chip still gets a few thousand wave-sized pieces (any value gives the
  // same integers)
  A.gw = 64;
  while (A.gw > 4 && (int64_t)batch * rg::ceil_div(A.W, A.gw) < 8192) A.gw >>= 1;
  A.n_groups = (int)rg::ceil_div(A.W, A.gw);
  const int per_query = (int)std::min<int64_t>(rg::ceil_div(A.n_groups, PF_WAVES), std::max<int64_t>(1, rg::ceil_div(4096, batch)));
  size_t lds_bins = (size_t)A.R * ((size_t)ap * 4 + (DIR ? 36 : 12)), lds_fixed = PF_LIST_BYTES, lds_max = PF_LDS_MAX;
  if constexpr (LAG) {       // n_rela_rows * (4 * ap + 12 * n_bins) beside the head list and the lag table in 80 KiB
    lds_bins = (size_t)A.R * ((size_t)ap * 4 + 12 * (size_t)x->n_bins); lds_fixed += (size_t)x->n_lag; lds_max = XPF_LDS_MAX;
  }
  const bool lds = lds_fixed + lds_bins <= lds_max;
  const size_t smem = lds_fixed + (lds ? lds_bins : 0);
  hipStream_t s = (hipStream_t)stream;
  return rg::with_ap4(ap / 4, who, [&](auto ap4) {
    constexpr int AP4 = decltype(ap4)::value;
    if constexpr (LAG) {     // (only this mode asks for more than the default 64 KB of dynamic LDS)
      if (smem > PF_LDS_MAX)
        RG_HIP(hipFuncSetAttribute((const void*)profile_kernel<AP4, true, DIR, LAG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    }
    if (lds) hipLaunchKernelGGL((profile_kernel<AP4, true, DIR, LAG>), dim3(per_query, batch), dim3(PF_BLOCK), smem, s, A);
    else hipLaunchKernelGGL((profile_kernel<AP4, false, DIR, LAG>), dim3(per_query, batch), dim3(PF_BLOCK), smem, s, A);
    RG_LAUNCH_CHECK();
    return 0;
  });
}

}  // namespace

extern "C" {

int rg_attn_profile(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                    const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                    int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream) {
  return profile_hop<false>("rg_attn_profile", f, g, batch, n_ent, level, n_old, nullptr, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim,
                            sum_out, count_out, stream);
}

int rg_tattn_profile(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                     const int32_t* q_time, const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                     const float* b_alpha, int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream) {
  return profile_hop<true>("rg_tattn_profile", f, g, batch, n_ent, level, n_old, q_time, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim,
                           sum_out, count_out, stream);
}

int rg_xattn_profile(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                     const int32_t* q_time, const int32_t* loop_time, const int32_t* row_time, const uint8_t* lag_bin, int32_t n_lag,
                     int32_t n_bins, const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                     const float* b_alpha, int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream) {
  const LagTable x{loop_time, row_time, lag_bin, n_lag, n_bins};
  return profile_hop<false, true>("rg_xattn_profile", f, g, batch, n_ent, level, n_old, q_time, a_s, a_r, a_q, ap, w_alpha, b_alpha,
                                  attn_dim, sum_out, count_out, stream, &x);
}

}  // extern "C"
