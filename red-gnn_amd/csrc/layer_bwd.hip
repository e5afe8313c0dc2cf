// Static RED-GNN entry point of the fused layer backward (the source-pull kernel: layer_bwd_kernel.h), and the relation-major
// pass behind its relation gradient.
#include "aq_sum.h"
#include "layer_bwd_kernel.h"

namespace rgbwd {
namespace {

// ---- relation gradient, relation-major --------------------------------------------------------------------------
// dRel[r] = sum over queries b and KG edges (h, r, t) with (b,h) in the previous frontier of alpha * G[(b,t)].
// Items are (query, 128-edge segment of relation r's edge list): the segment's sum is built in registers exactly as
// the forward kernel builds a destination row (test + rank + attention per candidate lane, then row gathers of G), and
// added to the workgroup's LDS copy of dRel ONCE per segment - 1/128th of the LDS float atomics of the per-edge form,
// which were two thirds of the backward kernel's time.
struct DrelArgs {
  rg::WalkArgs walk;          // vrows = CSR-by-relation segments; always live
  const int2* rel_ht;
  const int2* bm_old;
  const int2* bm_new;
  int W;
  const float4* a_s;
  const float4* a_r;
  const float4* a_q;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  int n_rela_rows;
  int ld4;
  const float4* grad_agg;
  float* g_rela;
};

// TABLE: the relation gradient is accumulated in an LDS copy of the table (one LDS row add per segment, one global add per
// block and row at the end).  When the table does not fit LDS (FB15k-237-like: 475 rows x 128) every segment's sum goes
// straight to global memory: still one row add per <= 128 edges.
template <int G, int AP4, bool TABLE>
__global__ __launch_bounds__(BWD_BLOCK, 4) void drel_kernel(DrelArgs A) {
  extern __shared__ float4 lds[];
  constexpr int BLOCK = BWD_BLOCK;
  // the LDS table is component-major inside a row and its rows are 8 floats apart in bank space: the 16 lanes of a group add to
  // 16 consecutive banks and four groups working on four different relations do not collide (ds_add_f32, 32 banks)
  constexpr int RS = 4 * G + 8;
  const int nr = A.n_rela_rows;
  float4* stage = lds;                                   // [BLOCK] {o, alpha}
  float4* ar_l = stage + BLOCK;                          // [nr][AP4]
  float4* w_l = ar_l + nr * AP4;                         // [AP4]
  float* table_l = reinterpret_cast<float*>(w_l + AP4);  // [nr][RS]  (TABLE)
  for (int i = threadIdx.x; i < nr * AP4; i += BLOCK) ar_l[i] = A.a_r[i];
  if (threadIdx.x < AP4) {
    float w[4];
    for (int k = 0; k < 4; ++k) {
      const int j = threadIdx.x * 4 + k;
      w[k] = j < A.attn_dim ? A.w_alpha[j] : 0.f;
    }
    w_l[threadIdx.x] = make_float4(w[0], w[1], w[2], w[3]);
  }
  if constexpr (TABLE) { for (int i = threadIdx.x; i < nr * RS; i += BLOCK) table_l[i] = 0.f; }
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
    const int beg = R.x, end = R.x + rg::walk_len(R), b = R.z, r = R.w;
    const int2* old_row = A.bm_old + (int64_t)b * A.W;
    const int2* new_row = A.bm_new + (int64_t)b * A.W;
    float4 base[AP4];
#pragma unroll
    for (int k = 0; k < AP4; ++k) {
      const float4 ar = ar_l[(live ? r : 0) * AP4 + k];
      const float4 aq = A.a_q[(int64_t)b * AP4 + k];
      base[k] = make_float4(ar.x + aq.x, ar.y + aq.y, ar.z + aq.z, ar.w + aq.w);
    }
    float4 acc = rg::f4zero();
    bool any = false;
    for (int c0 = beg; c0 < end; c0 += G) {
      const int c = c0 + lane_g;
      bool valid = c < end;
      int o = 0;
      float alpha = 0.f;
      if (valid) {
        const int2 ht = A.rel_ht[c];
        const int2 wp = old_row[ht.x >> 5];
        const uint32_t word = (uint32_t)wp.x, bit = ht.x & 31;
        valid = (word >> bit) & 1u;
        if (valid) {
          const int s = wp.y + __popc(word & ((1u << bit) - 1u));
          const int2 wn = new_row[ht.y >> 5];
          o = wn.y + __popc((uint32_t)wn.x & ((1u << (ht.y & 31)) - 1u));
          float z = b_alpha;
#pragma unroll
          for (int k = 0; k < AP4; ++k) {
            const float4 as = A.a_s[(int64_t)s * AP4 + k];
            const float4 w = w_l[k];
            z = fmaf(w.x, fmaxf(as.x + base[k].x, 0.f), z);
            z = fmaf(w.y, fmaxf(as.y + base[k].y, 0.f), z);
            z = fmaf(w.z, fmaxf(as.z + base[k].z, 0.f), z);
            z = fmaf(w.w, fmaxf(as.w + base[k].w, 0.f), z);
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
      if (valid) my_stage[pos] = make_float4(__int_as_float(o), alpha, 0.f, 0.f);
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      any = any || cnt > 0;
      for (int k = 0; k < cnt; k += 4) {
        float4 tp[4], gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tp[u] = my_stage[k + u];
#pragma unroll
        for (int u = 0; u < 4; ++u) gv[u] = A.grad_agg[(int64_t)__float_as_int(tp[u].x) * A.ld4 + lane_c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float al = tp[u].y;
          acc.x = fmaf(al, gv[u].x, acc.x);
          acc.y = fmaf(al, gv[u].y, acc.y);
          acc.z = fmaf(al, gv[u].z, acc.z);
          acc.w = fmaf(al, gv[u].w, acc.w);
        }
      }
    }
    if (live && any && row_lane) {
      if constexpr (TABLE) {
        float* gr = table_l + r * RS + lane_g;
        atomicAdd(gr, acc.x); atomicAdd(gr + G, acc.y); atomicAdd(gr + 2 * G, acc.z); atomicAdd(gr + 3 * G, acc.w);
      } else {
        float* gr = A.g_rela + ((int64_t)r * A.ld4 + lane_g) * 4;
        atomicAdd(gr + 0, acc.x); atomicAdd(gr + 1, acc.y); atomicAdd(gr + 2, acc.z); atomicAdd(gr + 3, acc.w);
      }
    }
  });

  if constexpr (TABLE) {
    __syncthreads();
    for (int i = threadIdx.x; i < nr * A.ld4 * 4; i += BLOCK) {
      const int r = i / (A.ld4 * 4), c = i - r * (A.ld4 * 4);
      const float v = table_l[r * RS + (c & 3) * G + (c >> 2)];
      if (v != 0.f) atomicAdd(A.g_rela + i, v);
    }
  }
}


template <int G, int AP4, bool TABLE>
int launch_drel(const DrelArgs& A, size_t lds, hipStream_t s) {
  RG_CHECK(lds <= 160 * 1024, "rg_layer_bwd: attention table needs %zu B of LDS (> 160 KiB)", lds);
  auto kern = drel_kernel<G, AP4, TABLE>;
  if (lds > 64 * 1024) RG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int grid = rg::walk_grid(A.walk.n_items, BWD_BLOCK, G, true, lds <= 80 * 1024 ? 2 : 1, 1);
  if (rg::zero_async(A.walk.queues, RG_QUEUE_BYTES, s)) return 1;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(BWD_BLOCK), lds, s, A);
  RG_LAUNCH_CHECK();
  return 0;
}

int launch_drel(const DrelArgs& A, int ap4, hipStream_t s) {
  return rg::with_g(A.ld4, [&](auto g) {
    return rg::with_ap4(ap4, "rg_layer_bwd", [&](auto ap) {
      constexpr int G = decltype(g)::value, AP4 = decltype(ap)::value;
      const size_t lds = (size_t)(BWD_BLOCK + A.n_rela_rows * AP4 + AP4) * sizeof(float4);
      const size_t table = (size_t)A.n_rela_rows * (4 * G + 8) * sizeof(float);
      return lds + table <= 80 * 1024 ? launch_drel<G, AP4, true>(A, lds + table, s) : launch_drel<G, AP4, false>(A, lds, s);
    });
  });
}

}  // namespace
}  // namespace rgbwd

extern "C" size_t rg_layer_bwd_scratch_bytes(const rg_frontier* f, const rg_graph* g, int32_t ld, int32_t ap) {
  if (!f || !g) return 0;
  return (size_t)f->B * g->out_vr.n_slots * (ld + ap) * sizeof(float) + 512;
}

extern "C" int rg_layer_bwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, const float* hidden,
                            const float* rela, int32_t d, int32_t ld, const float* a_s, const float* a_r,
                            const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                            const float* grad_agg, float* grad_hidden, float* grad_rela, float* grad_a_s,
                            float* grad_a_r, float* grad_a_q, float* grad_w_alpha, float* grad_b_alpha, void* scratch,
                            size_t scratch_bytes, void* stream) {
  RG_CHECK(f && g && hidden && rela && a_s && a_r && a_q && w_alpha && b_alpha && grad_agg && grad_hidden && grad_rela &&
               grad_a_s && grad_a_r && grad_w_alpha && grad_b_alpha, "rg_layer_bwd: NULL argument");
  if (rgbwd::check_common("rg_layer_bwd", f, g, level, n_old, d, ld, ap, attn_dim, scratch, scratch_bytes,
                          rg_layer_bwd_scratch_bytes(f, g, ld, ap))) return 1;
  if (n_old == 0) return grad_a_q ? rg::launch_aq_sum(f->bm_of(level - 1), f->W, f->B, f->n_ent, 0, grad_a_s, ap, grad_a_q, (hipStream_t)stream) : 0;
  rgbwd::BwdArgs A;
  rgbwd::fill_common(f, g, level, ld, 1, scratch, &A);
  A.out_pk = g->out_pk;
  A.hidden = (const float4*)hidden; A.rela = (const float4*)rela;
  A.a_s = (const float4*)a_s; A.a_r = (const float4*)a_r; A.a_q = (const float4*)a_q;
  A.w_alpha = w_alpha; A.b_alpha = b_alpha; A.attn_dim = attn_dim;
  A.grad_agg = (const float4*)grad_agg; A.g_hidden = (float4*)grad_hidden;
  A.g_as = (float4*)grad_a_s; A.g_ar = grad_a_r; A.g_w = grad_w_alpha; A.g_b = grad_b_alpha;
  A.kpg = rg::walk_kpg(g->n_fact, g->out_vr.n);
  hipStream_t s = (hipStream_t)stream;
  // every hop but the first walks densely: a sparse source set still carries hub rows of thousands of edges, and the
  // 64-items-per-lane filter of the sparse walk hands them to a few workgroups (measured 10x slower on C2 hop 1)
  const bool dense = n_old >= 4 * (int64_t)f->B;
  const int2* bm_old = f->bm_of(level - 1);
  if (rgbwd::launch<rgbwd::STATIC>("rg_layer_bwd", A, ap / 4, f->B, g->out_vr, bm_old, dense, s)) return 1;
  if (grad_a_q && rg::launch_aq_sum(bm_old, f->W, f->B, f->n_ent, n_old, grad_a_s, ap, grad_a_q, s)) return 1;
  // relation gradient, relation-major (see drel_kernel)
  rgbwd::DrelArgs D;
  D.walk.n_items = (int64_t)f->B * g->rel_vr.n; D.walk.n_vrows = g->rel_vr.n; D.walk.n_slots = 0; D.walk.vrows = g->rel_vr.rows;
  D.walk.bm_test = nullptr; D.walk.W = f->W; D.walk.queues = f->queues; f->queues_clean = false;
  RG_CHECK(D.walk.n_items / 8 + ((int64_t)1 << 26) < ((int64_t)1 << 31), "rg_layer_bwd: relation work space too large for 32-bit queue tickets");
  D.rel_ht = g->rel_ht; D.bm_old = bm_old; D.bm_new = f->bm_of(level); D.W = f->W;
  D.a_s = (const float4*)a_s; D.a_r = (const float4*)a_r; D.a_q = (const float4*)a_q;
  D.w_alpha = w_alpha; D.b_alpha = b_alpha; D.attn_dim = attn_dim; D.n_rela_rows = g->n_rela_rows; D.ld4 = ld / 4;
  D.grad_agg = (const float4*)grad_agg; D.g_rela = grad_rela;
  return rgbwd::launch_drel(D, ap / 4, s);
}
