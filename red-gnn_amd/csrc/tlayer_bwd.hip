// Temporal entry points of the fused layer backward (the source-pull kernel: layer_bwd_kernel.h): rg_tlayer_bwd, the adjoint
// of rg_tlayer_fwd (T-RED-GNN interpolation), and rg_xlayer_bwd, the adjoint of rg_xlayer_fwd (extrapolation: per-query row
// windows, one direction; hidden_dir / rela_dir / time_dir are then hidden_p [N_old] / rela_p / time_p [n_time]).
//   d hidden_dir[3 s + dir] += alpha G[o]      (layer_bwd_kernel: three register accumulators per source, one store per row)
//   d rela_dir / d time_dir rows += alpha G[o] (separate key-major passes, tkey_kernel: items are 128-edge segments of one
//                                               relation / one time id, so a whole segment lands in at most three rows / one row
//                                               and is added once; per-edge float atomics on a 2.5 k-row table cost 20x the forward)
// The direction linears and the attention's three blocks are differentiated by the caller (dense GEMMs).
#include "aq_sum.h"
#include "layer_bwd_kernel.h"

namespace rgbwd {
namespace {

// ---- table gradients, key-major -------------------------------------------------------------------------------------------
// BY_TIME = false: items = (query, segment of relation r's edge list); an edge's direction follows from its time id, so the
//                  segment's alpha*G sums go to up to three rows  dir * n_rela_rows + r  of g_rela_dir.
// BY_TIME = true : items = (query, segment of time id tau's edge list); dt = tau - q_time[b] is the same for the whole segment,
//                  which therefore lands in the single row  dir * n_time + |dt|  of g_time_dir.
struct TKeyArgs {
  rg::WalkArgs walk;          // vrows = CSR-by-relation / CSR-by-time segments; always live
  const int2* ht;             // {head, tail} per entry
  const int32_t* aux;         // BY_TIME ? relation : time id, per entry
  const int32_t* q_time;
  const int2* bm_old;
  const int2* bm_new;
  int W;
  const float4* a_s;
  const float4* a_r;
  const float4* a_q;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim, n_rela_rows, n_time, ld4;
  const float4* grad_agg;
  float* g_table;             // g_rela_dir or g_time_dir
  // WIN
  const int32_t* win_lo = nullptr;
  const int32_t* win_hi = nullptr;
  const int32_t* row_time = nullptr;
  const int32_t* loop_time = nullptr;
  int n_data = 0;
};

template <int G, int AP4, bool BY_TIME, bool WIN>
__global__ __launch_bounds__(BWD_BLOCK, 4) void tkey_kernel(TKeyArgs A) {
  extern __shared__ float4 lds[];
  constexpr int BLOCK = BWD_BLOCK;
  const int nr = A.n_rela_rows;
  float4* stage = lds;                // [BLOCK] {o, alpha, dir}
  float4* ar_l = stage + BLOCK;       // [nr][AP4]
  float4* w_l = ar_l + nr * AP4;      // [AP4]
  for (int i = threadIdx.x; i < nr * AP4; i += BLOCK) ar_l[i] = A.a_r[i];
  if (threadIdx.x < AP4) {
    float w[4];
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x * 4 + k;
      w[k] = j < A.attn_dim ? A.w_alpha[j] : 0.f;
    }
    w_l[threadIdx.x] = make_float4(w[0], w[1], w[2], w[3]);
  }
  __syncthreads();
  const float b_alpha = A.b_alpha[0];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lane_g = lane & (G - 1), gi_w = lane / G;
  float4* my_stage = stage + wv * 64 + gi_w * G;
  const int gshift = lane & ~(G - 1);
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const bool row_lane = lane_g < A.ld4;
  const int lane_c = row_lane ? lane_g : A.ld4 - 1;

  rg::walk_items<G, true, 1, BLOCK, true>(A.walk, nullptr, [&](const int4& R, bool live) {
    const int beg = R.x, b = R.z, key = R.w;
    int end = R.x + rg::walk_len(R);
    int wlo = 0, whi = 0;
    if constexpr (WIN) {
      wlo = A.win_lo[b]; whi = A.win_hi[b];
      if (BY_TIME && key < A.n_data && (key < wlo || key >= whi)) end = beg;      // the whole row lies outside the query's window
    }
    const int2* old_row = A.bm_old + (int64_t)b * A.W;
    const int2* new_row = A.bm_new + (int64_t)b * A.W;
    const int qt = A.q_time[b];
    float4 aq[AP4];
#pragma unroll
    for (int k = 0; k < AP4; ++k) aq[k] = A.a_q[(int64_t)b * AP4 + k];
    float4 acc[BY_TIME ? 1 : 3];
#pragma unroll
    for (int dd = 0; dd < (BY_TIME ? 1 : 3); ++dd) acc[dd] = rg::f4zero();
    unsigned seen = 0u;      // directions with at least one edge (BY_TIME: bit 0)
    for (int c0 = beg; c0 < end; c0 += G) {
      const int c = c0 + lane_g;
      bool valid = c < end;
      int o = 0, dir = 0;
      float alpha = 0.f;
      if (valid) {
        const int2 ht = A.ht[c];
        const int2 wp = old_row[ht.x >> 5];
        const uint32_t word = (uint32_t)wp.x, bit = ht.x & 31;
        valid = (word >> bit) & 1u;
        if constexpr (WIN && !BY_TIME) {
          if (valid) { const int erow = A.aux[c]; valid = erow >= A.n_data || (erow >= wlo && erow < whi); }
        }
        if (valid) {
          const int s = wp.y + __popc(word & ((1u << bit) - 1u));
          const int2 wn = new_row[ht.y >> 5];
          o = wn.y + __popc((uint32_t)wn.x & ((1u << (ht.y & 31)) - 1u));
          const int other = A.aux[c];
          const int r = BY_TIME ? other : key;
          if constexpr (!BY_TIME && !WIN) { const int dt = other - qt; dir = dt > 0 ? 2 : (dt == 0 ? 1 : 0); }
          float z = b_alpha;
#pragma unroll
          for (int k = 0; k < AP4; ++k) {
            const float4 as = A.a_s[(int64_t)s * AP4 + k];
            const float4 ar = ar_l[r * AP4 + k];
            const float4 w = w_l[k];
            z = fmaf(w.x, fmaxf(as.x + ar.x + aq[k].x, 0.f), z);
            z = fmaf(w.y, fmaxf(as.y + ar.y + aq[k].y, 0.f), z);
            z = fmaf(w.z, fmaxf(as.z + ar.z + aq[k].z, 0.f), z);
            z = fmaf(w.w, fmaxf(as.w + ar.w + aq[k].w, 0.f), z);
          }
          alpha = __builtin_amdgcn_rcpf(1.0f + __expf(-z));
        }
      }
      const unsigned long long m = (__ballot(valid) >> gshift) & gmask;
      const int cnt = __popcll(m);
      const int pos = __popcll(m & ((1ull << lane_g) - 1ull));
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      if (lane_g >= cnt) my_stage[lane_g] = rg::f4zero();
      if (valid) my_stage[pos] = make_float4(__int_as_float(o), alpha, __int_as_float(dir), 0.f);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      for (int k = 0; k < cnt; k += 4) {
        float4 tp[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tp[u] = my_stage[k + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = A.grad_agg[(int64_t)__float_as_int(tp[u].x) * A.ld4 + lane_c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float al = tp[u].y;
          if constexpr (BY_TIME) {
            acc[0].x = fmaf(al, gv[u].x, acc[0].x); acc[0].y = fmaf(al, gv[u].y, acc[0].y);
            acc[0].z = fmaf(al, gv[u].z, acc[0].z); acc[0].w = fmaf(al, gv[u].w, acc[0].w);
            if (k + u < cnt) seen |= 1u;
          } else {
            const int du = __float_as_int(tp[u].z);
#pragma unroll
            for (int dd = 0; dd < 3; ++dd) {
              const float mk = du == dd ? al : 0.f;
              acc[dd].x = fmaf(mk, gv[u].x, acc[dd].x); acc[dd].y = fmaf(mk, gv[u].y, acc[dd].y);
              acc[dd].z = fmaf(mk, gv[u].z, acc[dd].z); acc[dd].w = fmaf(mk, gv[u].w, acc[dd].w);
            }
            if (k + u < cnt) seen |= 1u << du;
          }
        }
      }
    }
    if (live && row_lane) {
      if constexpr (BY_TIME) {
        if (seen) {
          int trow;
          if constexpr (WIN) {
            trow = min(max(qt - (key >= A.n_data ? A.loop_time[b] : A.row_time[key]), 0), A.n_time - 1);
          } else {
            const int dt = key - qt;
            const int dir = dt > 0 ? 2 : (dt == 0 ? 1 : 0);
            trow = dir * A.n_time + (dt < 0 ? -dt : dt);
          }
          float* gr = A.g_table + ((int64_t)trow * A.ld4 + lane_g) * 4;
          atomicAdd(gr + 0, acc[0].x); atomicAdd(gr + 1, acc[0].y); atomicAdd(gr + 2, acc[0].z); atomicAdd(gr + 3, acc[0].w);
        }
      } else {
#pragma unroll
        for (int dd = 0; dd < (WIN ? 1 : 3); ++dd)
          if (seen & (1u << dd)) {
            float* gr = A.g_table + ((int64_t)(dd * nr + key) * A.ld4 + lane_g) * 4;
            atomicAdd(gr + 0, acc[dd].x); atomicAdd(gr + 1, acc[dd].y); atomicAdd(gr + 2, acc[dd].z); atomicAdd(gr + 3, acc[dd].w);
          }
      }
    }
  });
}

template <bool BY_TIME>
int launch_tkey(const char* who, const TKeyArgs& A, int ap4, hipStream_t s) {
  return rg::with_g(A.ld4, [&](auto g) {
    return rg::with_ap4(ap4, who, [&](auto ap) {
      constexpr int G = decltype(g)::value, AP4 = decltype(ap)::value;
      const size_t lds = (size_t)(BWD_BLOCK + A.n_rela_rows * AP4 + AP4) * sizeof(float4);
      RG_CHECK(lds <= 160 * 1024, "%s: attention table needs %zu B of LDS (> 160 KiB)", who, lds);
      auto kern = A.win_lo ? tkey_kernel<G, AP4, BY_TIME, true> : tkey_kernel<G, AP4, BY_TIME, false>;
      if (lds > 64 * 1024) RG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const int grid = rg::walk_grid(A.walk.n_items, BWD_BLOCK, G, true, lds <= 80 * 1024 ? 2 : 1, 1);
      if (rg::zero_async(A.walk.queues, RG_QUEUE_BYTES, s)) return 1;
      hipLaunchKernelGGL(kern, dim3(grid), dim3(BWD_BLOCK), lds, s, A);
      RG_LAUNCH_CHECK();
      return 0;
    });
  });
}

struct WinArgs {            // the extrapolation setting's extras; all null / 0 for the interpolation layer
  const int32_t* loop_time = nullptr;
  const int32_t* row_time = nullptr;
  int n_data = 0, n_tab = 0;
};

int tbwd_impl(const char* who, const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, const int32_t* q_time,
              const float* hidden_dir, const float* rela_dir, const float* time_dir, int32_t d, int32_t ld,
              const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
              const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_hidden_dir,
              float* grad_rela_dir, float* grad_time_dir, float* grad_a_s, float* grad_a_r,
              float* grad_a_q, float* grad_w_alpha, void* scratch, size_t scratch_bytes, const WinArgs& win, void* stream) {
  const bool windowed = win.row_time != nullptr;
  RG_CHECK(f && g && q_time && hidden_dir && rela_dir && time_dir && a_s && a_r && a_q && w_alpha && b_alpha && grad_agg &&
               grad_hidden_dir && grad_rela_dir && grad_time_dir && grad_a_s && grad_a_r && grad_w_alpha,
           "%s: NULL argument", who);
  RG_CHECK(g->out_time && g->rel_tm && g->time_ht && g->n_time > 0, "%s: the graph has no timestamps (build it with rg_tgraph_create)", who);
  RG_CHECK((int64_t)f->B * f->n_ent * 3 < ((int64_t)1 << 31), "%s: 3 * batch * n_ent does not fit int32 row ids", who);
  const int n_time = windowed ? win.n_tab : g->n_time;
  RG_CHECK((int64_t)3 * n_time * 4 + 3 < ((int64_t)1 << 31), "%s: n_time too large", who);
  RG_CHECK(!windowed || (f->win_lo && f->win_hi && win.loop_time && win.n_tab > 0 && win.n_data >= 0),
           "%s: call rg_frontier_set_window first (and pass loop_time, n_tab)", who);
  if (check_common(who, f, g, level, n_old, d, ld, ap, attn_dim, scratch, scratch_bytes, rg_tlayer_bwd_scratch_bytes(f, g, ld, ap)))
    return 1;
  if (n_old == 0) return grad_a_q ? rg::launch_aq_sum(f->bm_of(level - 1), f->W, f->B, f->n_ent, 0, grad_a_s, ap, grad_a_q, (hipStream_t)stream) : 0;
  BwdArgs A;
  fill_common(f, g, level, ld, windowed ? 1 : 3, scratch, &A);
  A.hidden = (const float4*)hidden_dir; A.rela = (const float4*)rela_dir;
  A.a_s = (const float4*)a_s; A.a_r = (const float4*)a_r; A.a_q = (const float4*)a_q;
  A.w_alpha = w_alpha; A.b_alpha = b_alpha; A.attn_dim = attn_dim;
  A.grad_agg = (const float4*)grad_agg; A.g_hidden = (float4*)grad_hidden_dir;
  A.g_as = (float4*)grad_a_s; A.g_ar = grad_a_r; A.g_w = grad_w_alpha;
  A.out_time = g->out_time; A.q_time = q_time; A.time_tab = (const float4*)time_dir; A.n_time = n_time;
  if (windowed) { A.win_lo = f->win_lo; A.win_hi = f->win_hi; A.row_time = win.row_time; A.loop_time = win.loop_time; A.n_data = win.n_data; }
  hipStream_t s = (hipStream_t)stream;
  const bool dense = n_old >= 4 * (int64_t)f->B;
  const int2* bm_old = f->bm_of(level - 1);
  if (windowed ? launch<WINDOWED>(who, A, ap / 4, f->B, g->out_vr, bm_old, dense, s)
               : launch<TEMPORAL>(who, A, ap / 4, f->B, g->out_vr, bm_old, dense, s)) return 1;
  if (grad_a_q && rg::launch_aq_sum(bm_old, f->W, f->B, f->n_ent, n_old, grad_a_s, ap, grad_a_q, s)) return 1;
  // table gradients, key-major (see tkey_kernel)
  TKeyArgs K;
  K.q_time = q_time; K.bm_old = bm_old; K.bm_new = f->bm_of(level); K.W = f->W;
  K.a_s = (const float4*)a_s; K.a_r = (const float4*)a_r; K.a_q = (const float4*)a_q;
  K.w_alpha = w_alpha; K.b_alpha = b_alpha; K.attn_dim = attn_dim; K.n_rela_rows = g->n_rela_rows; K.n_time = n_time; K.ld4 = ld / 4;
  K.grad_agg = (const float4*)grad_agg;
  if (windowed) { K.win_lo = f->win_lo; K.win_hi = f->win_hi; K.row_time = win.row_time; K.loop_time = win.loop_time; K.n_data = win.n_data; }
  K.walk.n_slots = 0; K.walk.bm_test = nullptr; K.walk.W = f->W; K.walk.queues = f->queues; f->queues_clean = false;
  K.walk.n_items = (int64_t)f->B * g->rel_vr.n; K.walk.n_vrows = g->rel_vr.n; K.walk.vrows = g->rel_vr.rows;
  RG_CHECK(K.walk.n_items / 8 + ((int64_t)1 << 26) < ((int64_t)1 << 31), "%s: relation work space too large for 32-bit queue tickets", who);
  K.ht = g->rel_ht; K.aux = g->rel_tm; K.g_table = grad_rela_dir;
  if (launch_tkey<false>(who, K, ap / 4, s)) return 1;
  K.walk.n_items = (int64_t)f->B * g->time_vr.n; K.walk.n_vrows = g->time_vr.n; K.walk.vrows = g->time_vr.rows;
  RG_CHECK(K.walk.n_items / 8 + ((int64_t)1 << 26) < ((int64_t)1 << 31), "%s: time work space too large for 32-bit queue tickets", who);
  K.ht = g->time_ht; K.aux = g->time_rel; K.g_table = grad_time_dir;
  return launch_tkey<true>(who, K, ap / 4, s);
}

}  // namespace
}  // namespace rgbwd

extern "C" size_t rg_tlayer_bwd_scratch_bytes(const rg_frontier* f, const rg_graph* g, int32_t ld, int32_t ap) {
  if (!f || !g) return 0;
  return (size_t)f->B * g->out_vr.n_slots * (3 * ld + ap) * sizeof(float) + 512;
}

extern "C" int rg_tlayer_bwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, const int32_t* q_time,
                             const float* hidden_dir, const float* rela_dir, const float* time_dir, int32_t d, int32_t ld,
                             const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                             const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_hidden_dir,
                             float* grad_rela_dir, float* grad_time_dir, float* grad_a_s, float* grad_a_r,
                             float* grad_a_q, float* grad_w_alpha, void* scratch, size_t scratch_bytes, void* stream) {
  return rgbwd::tbwd_impl("rg_tlayer_bwd", f, g, level, n_old, q_time, hidden_dir, rela_dir, time_dir, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha,
                   attn_dim, grad_agg, grad_hidden_dir, grad_rela_dir, grad_time_dir, grad_a_s, grad_a_r, grad_a_q, grad_w_alpha, scratch,
                   scratch_bytes, rgbwd::WinArgs(), stream);
}

// Adjoint of rg_xlayer_fwd (temporal extrapolation; see the header comment): grad_hidden_p [N_old, ld], grad_rela_p [n_rela_rows, ld],
// grad_time_p [n_tab, ld] (the last two zero-initialised by the caller, added into), the attention gradients as rg_tlayer_bwd.
extern "C" int rg_xlayer_bwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, const int32_t* q_time,
                             const int32_t* loop_time, const int32_t* row_time, int32_t n_data, const float* hidden_p, const float* rela_p,
                             const float* time_p, int32_t n_tab, int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q,
                             int32_t ap, const float* w_alpha, const float* b_alpha, int32_t attn_dim, const float* grad_agg,
                             float* grad_hidden_p, float* grad_rela_p, float* grad_time_p, float* grad_a_s, float* grad_a_r, float* grad_a_q,
                             float* grad_w_alpha, void* scratch, size_t scratch_bytes, void* stream) {
  RG_CHECK(loop_time && row_time, "rg_xlayer_bwd: NULL argument");
  rgbwd::WinArgs w;
  w.loop_time = loop_time; w.row_time = row_time; w.n_data = n_data; w.n_tab = n_tab;
  return rgbwd::tbwd_impl("rg_xlayer_bwd", f, g, level, n_old, q_time, hidden_p, rela_p, time_p, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim,
                   grad_agg, grad_hidden_p, grad_rela_p, grad_time_p, grad_a_s, grad_a_r, grad_a_q, grad_w_alpha, scratch, scratch_bytes, w, stream);
}
