// Table gradients of the fused layer backward, key-major: the relation table's (every layer) and the time table's (temporal
// layers), one kernel for all of them.  layer_bwd_kernel.h's source-pull walk would add a row per EDGE to these tables with float
// atomics (two thirds of the static backward's time; 20x the forward on the temporal layers' 2.5 k-row tables).  Here
//   items = (query b, 128-edge segment of ONE key's edge list)     key = relation (CSR by relation) or time id (CSR by time)
// so a whole segment's  sum of alpha * G[o]  is built in registers exactly as the forward builds a destination row - test + rank +
// attention per candidate lane (attn.h), ballot compaction, four row gathers of grad_agg in flight - and lands in one table row
// (three, by direction, for the temporal relation key), added ONCE per segment.
//
//   key       layer     accumulators                    row of the table the segment is added to
//   relation  STATIC    1 (a_r[r] + a_q[b] pre-summed)  r: in the workgroup's LDS copy of the table (TABLE; flushed per block and
//                                                       row at the end) or, where the table does not fit LDS (FB15k-237-like:
//                                                       475 rows x 128), straight in global memory
//   relation  TEMPORAL  3, by the edge's direction      dir * n_rela_rows + r     (dir from the edge's time id: aux - q_time[b])
//   relation  WINDOWED  1; edges outside [win_lo[b], win_hi[b]) by their data row (aux) are no edges      r
//   time      TEMPORAL  1                               dir * n_time + |dt|,  dt = key - q_time[b]: the same for the whole segment
//   time      WINDOWED  1; a data row outside the window skips the item      clamp(q_time[b] - row_time[key], 0, n_time - 1)
#pragma once
#include "layer_bwd_kernel.h"

namespace rgbwd {
namespace {

struct KeyArgs {
  rg::WalkArgs walk;          // vrows = CSR-by-relation / CSR-by-time segments; always live
  const int2* ht;             // {head, tail} per entry
  const int32_t* aux = nullptr;      // temporal layers: time id (data row) per entry of the CSR by relation, relation per entry of the CSR by time
  const int32_t* q_time = nullptr;   // temporal layers
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
  float* g_table;             // the relation table's or the time table's gradient, added into
  // WINDOWED
  const int32_t* win_lo = nullptr;
  const int32_t* win_hi = nullptr;
  const int32_t* row_time = nullptr;
  const int32_t* loop_time = nullptr;
  int n_data = 0;
};

template <int G, int AP4, Layer L, bool BY_TIME, bool TABLE>
__global__ __launch_bounds__(BWD_BLOCK, 4) void key_bwd_kernel(KeyArgs A) {
  static_assert(!(BY_TIME && L == STATIC) && !(TABLE && L != STATIC), "see the table of flavours");
  extern __shared__ float4 lds[];
  constexpr int BLOCK = BWD_BLOCK;
  constexpr int NA = (L == TEMPORAL && !BY_TIME) ? 3 : 1;
  // the LDS table is component-major inside a row and its rows are 8 floats apart in bank space: the 16 lanes of a group add to
  // 16 consecutive banks and four groups working on four different relations do not collide (ds_add_f32, 32 banks)
  constexpr int RS = 4 * G + 8;
  const int nr = A.n_rela_rows;
  float4* stage = lds;                                   // [BLOCK] {o, alpha, dir}
  float4* ar_l = stage + BLOCK;                          // [nr][AP4]
  float4* w_l = ar_l + nr * AP4;                         // [AP4]
  float* table_l = reinterpret_cast<float*>(w_l + AP4);  // [nr][RS]  (TABLE)
  rg::stage_attention<AP4, BLOCK>(ar_l, w_l, A.a_r, nr, A.w_alpha, A.attn_dim);
  if constexpr (TABLE) { for (int i = threadIdx.x; i < nr * RS; i += BLOCK) table_l[i] = 0.f; }
  __syncthreads();
  const float b_alpha = A.b_alpha[0];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lane_g = lane & (G - 1), gi_w = lane / G;
  float4* my_stage = stage + wv * 64 + gi_w * G;
  const bool row_lane = lane_g < A.ld4;
  const int lane_c = row_lane ? lane_g : A.ld4 - 1;

  rg::walk_items<G, true, 1, BLOCK, true>(A.walk, nullptr, [&](const int4& R, bool live) {
    const int beg = R.x, b = R.z, key = R.w;
    int end = R.x + rg::walk_len(R);
    int qt = 0, wlo = 0, whi = 0;
    if constexpr (L != STATIC) qt = A.q_time[b];
    if constexpr (L == WINDOWED) {
      wlo = A.win_lo[b]; whi = A.win_hi[b];
      if (BY_TIME && key < A.n_data && (key < wlo || key >= whi)) end = beg;      // the whole row lies outside the query's window
    }
    const int2* old_row = A.bm_old + (int64_t)b * A.W;
    const int2* new_row = A.bm_new + (int64_t)b * A.W;
    float4 base[AP4];      // the item's second attention operand: a_q[b], STATIC: a_r[r] + a_q[b] (attn.h on the orders)
#pragma unroll
    for (int k = 0; k < AP4; ++k) {
      if constexpr (L == STATIC) base[k] = rg::f4add(ar_l[(live ? key : 0) * AP4 + k], A.a_q[(int64_t)b * AP4 + k]);
      else base[k] = A.a_q[(int64_t)b * AP4 + k];
    }
    float4 acc[NA];
#pragma unroll
    for (int dd = 0; dd < NA; ++dd) acc[dd] = rg::f4zero();
    bool any = false;        // STATIC: the segment has an edge
    unsigned seen = 0u;      // temporal layers: the accumulators (directions) with an edge
    for (int c0 = beg; c0 < end; c0 += G) {
      const int c = c0 + lane_g;
      bool valid = c < end;
      int o = 0, dir = 0;
      float alpha = 0.f;
      if (valid) {
        const int2 ht = A.ht[c];
        const int2 wp = old_row[ht.x >> 5];
        valid = rg::bm_has(wp, ht.x);
        if constexpr (L == WINDOWED && !BY_TIME) {
          if (valid) { const int erow = A.aux[c]; valid = erow >= A.n_data || (erow >= wlo && erow < whi); }
        }
        if (valid) {
          const int s = rg::bm_rank(wp, ht.x);
          o = rg::bm_rank(new_row[ht.y >> 5], ht.y);
          int r = key;
          if constexpr (L != STATIC) {
            const int other = A.aux[c];
            if constexpr (BY_TIME) r = other;
            else if constexpr (L == TEMPORAL) { const int dt = other - qt; dir = dt > 0 ? 2 : (dt == 0 ? 1 : 0); }
          }
          float z = b_alpha;
#pragma unroll
          for (int k = 0; k < AP4; ++k) {
            const float4 as = A.a_s[(int64_t)s * AP4 + k];
            if constexpr (L == STATIC) rg::attn_acc(z, w_l[k], as, base[k]);
            else rg::attn_acc_fwd(z, w_l[k], as, ar_l[r * AP4 + k], base[k]);
          }
          alpha = rg::attn_alpha(z);
        }
      }
      const int cnt = rg::group_compact<G, true>(my_stage, lane, valid, make_float4(__int_as_float(o), alpha, __int_as_float(dir), 0.f));
      if constexpr (L == STATIC) any = any || cnt > 0;
      for (int k = 0; k < cnt; k += 4) {
        float4 tp[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tp[u] = my_stage[k + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = A.grad_agg[(int64_t)__float_as_int(tp[u].x) * A.ld4 + lane_c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float al = tp[u].y;
          const int du = NA == 1 ? 0 : __float_as_int(tp[u].z);
#pragma unroll
          for (int dd = 0; dd < NA; ++dd) {
            const float mk = (NA == 1 || du == dd) ? al : 0.f;
            acc[dd].x = fmaf(mk, gv[u].x, acc[dd].x); acc[dd].y = fmaf(mk, gv[u].y, acc[dd].y);
            acc[dd].z = fmaf(mk, gv[u].z, acc[dd].z); acc[dd].w = fmaf(mk, gv[u].w, acc[dd].w);
          }
          if constexpr (L != STATIC) { if (k + u < cnt) seen |= 1u << du; }
        }
      }
    }
    if (live && row_lane) {
#pragma unroll
      for (int dd = 0; dd < NA; ++dd) {
        if (L == STATIC ? !any : !(seen & (1u << dd))) continue;
        int row = dd * nr + key;
        if constexpr (BY_TIME && L == WINDOWED) {
          row = min(max(qt - (key >= A.n_data ? A.loop_time[b] : A.row_time[key]), 0), A.n_time - 1);
        } else if constexpr (BY_TIME) {
          const int dt = key - qt;
          row = (dt > 0 ? 2 : (dt == 0 ? 1 : 0)) * A.n_time + (dt < 0 ? -dt : dt);
        }
        if constexpr (TABLE) {
          float* gr = table_l + row * RS + lane_g;
          atomicAdd(gr, acc[dd].x); atomicAdd(gr + G, acc[dd].y); atomicAdd(gr + 2 * G, acc[dd].z); atomicAdd(gr + 3 * G, acc[dd].w);
        } else {
          float* gr = A.g_table + ((int64_t)row * A.ld4 + lane_g) * 4;
          atomicAdd(gr + 0, acc[dd].x); atomicAdd(gr + 1, acc[dd].y); atomicAdd(gr + 2, acc[dd].z); atomicAdd(gr + 3, acc[dd].w);
        }
      }
    }
  });

  if constexpr (TABLE) {
    __syncthreads();
    for (int i = threadIdx.x; i < nr * A.ld4 * 4; i += BLOCK) {
      const int r = i / (A.ld4 * 4), c = i - r * (A.ld4 * 4);
      const float v = table_l[r * RS + (c & 3) * G + (c >> 2)];
      if (v != 0.f) atomicAdd(A.g_table + i, v);
    }
  }
}

// the pass at the widths ld4 = A.ld4, ap4.  STATIC picks TABLE where the LDS copy of the table leaves two workgroups per CU.
template <Layer L, bool BY_TIME>
int launch_key(const char* who, const KeyArgs& A, int ap4, hipStream_t s) {
  return rg::with_g(A.ld4, [&](auto g) {
    return rg::with_ap4(ap4, who, [&](auto ap) {
      constexpr int G = decltype(g)::value, AP4 = decltype(ap)::value;
      size_t lds = (size_t)(BWD_BLOCK + A.n_rela_rows * AP4 + AP4) * sizeof(float4);
      auto kern = key_bwd_kernel<G, AP4, L, BY_TIME, false>;
      if constexpr (L == STATIC) {
        const size_t table = (size_t)A.n_rela_rows * (4 * G + 8) * sizeof(float);
        if (lds + table <= 80 * 1024) { lds += table; kern = key_bwd_kernel<G, AP4, L, BY_TIME, true>; }
      }
      RG_CHECK(lds <= 160 * 1024, "%s: attention table needs %zu B of LDS (> 160 KiB)", who, lds);
      if (lds > 64 * 1024) RG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      const int grid = rg::walk_grid(A.walk.n_items, BWD_BLOCK, G, true, lds <= 80 * 1024 ? 2 : 1, 1);
      if (rg::zero_async(A.walk.queues, RG_QUEUE_BYTES, s)) return 1;
      hipLaunchKernelGGL(kern, dim3(grid), dim3(BWD_BLOCK), lds, s, A);
      RG_LAUNCH_CHECK();
      return 0;
    });
  });
}

// KeyArgs of the pass over `vr` (g->rel_vr with rel_ht / rel_tm, g->time_vr with time_ht / time_rel; `what` names the key in the
// error message) for the layer whose source-pull arguments are B: the frontiers, attention tables and windows are B's.
inline int fill_key(const char* who, const char* what, const rg_frontier* f, const rg_vrows& vr, const int2* ht, const int32_t* aux,
                    const int2* bm_old, const BwdArgs& B, float* g_table, KeyArgs* K) {
  K->walk.n_items = (int64_t)f->B * vr.n; K->walk.n_vrows = vr.n; K->walk.n_slots = 0; K->walk.vrows = vr.rows;
  K->walk.bm_test = nullptr; K->walk.W = f->W; K->walk.queues = f->queues; f->queues_clean = false;
  RG_CHECK(K->walk.n_items / 8 + ((int64_t)1 << 26) < ((int64_t)1 << 31), "%s: %s work space too large for 32-bit queue tickets", who, what);
  K->ht = ht; K->aux = aux; K->q_time = B.q_time; K->bm_old = bm_old; K->bm_new = B.bm_new; K->W = B.W;
  K->a_s = B.a_s; K->a_r = B.a_r; K->a_q = B.a_q; K->w_alpha = B.w_alpha; K->b_alpha = B.b_alpha; K->attn_dim = B.attn_dim;
  K->n_rela_rows = B.n_rela_rows; K->n_time = B.n_time; K->ld4 = B.ld4; K->grad_agg = B.grad_agg; K->g_table = g_table;
  K->win_lo = B.win_lo; K->win_hi = B.win_hi; K->row_time = B.row_time; K->loop_time = B.loop_time; K->n_data = B.n_data;
  return 0;
}

}  // namespace
}  // namespace rgbwd
