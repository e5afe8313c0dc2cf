// Static RED-GNN entry point of the fused layer backward: the source-pull kernel (layer_bwd_kernel.h) and, for the relation
// gradient, the key-major pass over the CSR by relation (key_bwd_kernel.h, STATIC).
#include "aq_sum.h"
#include "key_bwd_kernel.h"

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
  // relation gradient, relation-major
  rgbwd::KeyArgs K;
  if (rgbwd::fill_key("rg_layer_bwd", "relation", f, g->rel_vr, g->rel_ht, nullptr, bm_old, A, grad_rela, &K)) return 1;
  return rgbwd::launch_key<rgbwd::STATIC, false>("rg_layer_bwd", K, ap / 4, s);
}
