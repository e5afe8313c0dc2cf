// Temporal entry points of the fused layer backward: rg_tlayer_bwd, the adjoint of rg_tlayer_fwd (T-RED-GNN interpolation), and
// rg_xlayer_bwd, the adjoint of rg_xlayer_fwd (extrapolation: per-query row windows, one direction; hidden_dir / rela_dir / time_dir
// are then hidden_p [N_old] / rela_p / time_p [n_time]).
//   d hidden_dir[3 s + dir] += alpha G[o]      (layer_bwd_kernel.h: three register accumulators per source, one store per row)
//   d rela_dir / d time_dir rows += alpha G[o] (key_bwd_kernel.h, TEMPORAL / WINDOWED: one pass keyed by relation, one by time id)
// The direction linears and the attention's three blocks are differentiated by the caller (dense GEMMs).
#include "aq_sum.h"
#include "key_bwd_kernel.h"

namespace rgbwd {
namespace {

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
  // table gradients, key-major: the relation table's over the CSR by relation, then the time table's over the CSR by time id
  KeyArgs K;
  if (fill_key(who, "relation", f, g->rel_vr, g->rel_ht, g->rel_tm, bm_old, A, grad_rela_dir, &K)) return 1;
  if (windowed ? launch_key<WINDOWED, false>(who, K, ap / 4, s) : launch_key<TEMPORAL, false>(who, K, ap / 4, s)) return 1;
  if (fill_key(who, "time", f, g->time_vr, g->time_ht, g->time_rel, bm_old, A, grad_time_dir, &K)) return 1;
  return windowed ? launch_key<WINDOWED, true>(who, K, ap / 4, s) : launch_key<TEMPORAL, true>(who, K, ap / 4, s);
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
