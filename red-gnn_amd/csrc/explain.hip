// Relational-digraph extraction: the edges of the query subgraph that the score of one answer depends on, with their attention.
//
// For a row (s, r, o) the r-digraph is the union of the length-L paths s -> o through the frontier's levels (identity edges count
// as steps).  It is found backwards from o, one hop at a time, over per-level mark bitmaps M_l in the frontier's batch-major word
// layout [B][W]:
//   M_L = {o} if o is in level L;  for l = L..1: the hop-l edges (h, rel, t) with t in M_l, h in level l-1 and alpha >= tau are
//   kept, and M_{l-1} = their heads.
// A hop is two passes of the same kernel over the words of M_l (one wave per 64 words; inside a word, marked entities in order,
// their CSR-by-tail rows in order, 64 in-edges at a time):
//   count: per-word edge counts (integers: placement cannot change them) and the heads' bits of M_{l-1} (non-returning atomicOr,
//          order-free);
//   emit:  after an exclusive scan of the counts, every kept edge is written at its word's offset + its rank among the word's
//          kept edges (ballot prefix): output order (row, tail, CSR position), deterministic.
// alpha is the forward kernel's arithmetic - the same attn.h calls in the forward's operand order, so the forward's alpha bit for
// bit - re-evaluated on the marked tails' in-edges only: nothing E_subgraph-sized is read or held.  A last gather puts the hops'
// lists into (row, hop, ...) order.
//
// Temporal graphs (rg_texplain_*, T-RED-GNN interpolation): the same walk over a quadruple graph.  The temporal attention does not
// read the edge's time, so the count pass IS the static instantiation; the emit pass is the kernel's TIME instantiation, which also
// writes the entry's time id (in_time[c]) beside the edge, so that a fact repeated at several times stays told apart.
//
// Extrapolation (rg_xexplain_*, the one-graph layout of extrapolation.py): in_time[c] is the edge's data row and the frontier carries
// the queries' row windows.  The WINDOW instantiation keeps an edge of query b only if its row is a self-loop (row >= n_data) or lies
// in [win_lo[b], win_hi[b]) - the forward's test (layer_fwd_kernel.h), needed in BOTH passes - and its emit pass writes the data row.
#include "attn.h"

namespace {

constexpr int EX_BLOCK = 256;

struct ExArgs {
  const uint32_t* marks;     // M_l [B][W]
  int64_t n_words;           // B * W
  int W;
  const int32_t* in_ptr;
  const int2* in_hr;
  const int2* bm_old;        // level l-1 {word, prefix}
  const float4* a_s;         // [N_{l-1}][ap4]
  const float4* a_r;         // [n_rela_rows][ap4]
  const float4* a_q;         // [B][ap4]
  int ap4;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  float tau;
  uint32_t* marks_prev;      // count: M_{l-1} (zeroed before)
  int32_t* word_count;       // count: kept edges per word of M_l
  const int32_t* word_ptr;   // emit: exclusive scan of word_count
  int4* edges;               // emit: (row, head, rel, tail)
  float* alpha;              // emit
};

__global__ void seed_kernel(const int2* __restrict__ bm_last, int B, int W, int n_ent, const int32_t* __restrict__ objs,
                            uint32_t* __restrict__ marks, uint8_t* __restrict__ reached) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int o = objs[b];
  bool ok = o >= 0 && o < n_ent;
  if (ok) ok = ((uint32_t)bm_last[(int64_t)b * W + (o >> 5)].x >> (o & 31)) & 1u;
  if (ok) marks[(int64_t)b * W + (o >> 5)] = 1u << (o & 31);     // one word per row: a plain store
  reached[b] = ok ? 1 : 0;
}

struct TExArgs : ExArgs {
  const int32_t* in_time;    // time id of every CSR-by-tail entry
  int32_t* time_out;         // emit: in_time[c] of every kept edge
};

struct XExArgs : TExArgs {   // in_time = data row of every CSR-by-tail entry
  const int32_t* win_lo;     // [B] first data row of the query's window
  const int32_t* win_hi;     // [B] one past its last
  int32_t n_data;            // rows >= n_data are the self-loops
};

template <bool EMIT, bool TIME = false, bool WINDOW = false>
__global__ __launch_bounds__(EX_BLOCK) void explain_kernel(
    std::conditional_t<WINDOW, XExArgs, std::conditional_t<TIME, TExArgs, ExArgs>> A) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = ((int64_t)blockIdx.x * (EX_BLOCK / 64) + (threadIdx.x >> 6)) * 64;
  if (w0 >= A.n_words) return;                       // (uniform over the wave)
  const int64_t wi = w0 + lane;
  const uint32_t my_word = wi < A.n_words ? A.marks[wi] : 0u;
  unsigned long long live = __ballot(my_word != 0u);
  int32_t my_count = 0;
  const float b_alpha = A.b_alpha[0];
  while (live) {
    const int j = __ffsll(live) - 1;
    live &= live - 1ull;
    const int64_t wj = w0 + j;
    uint32_t bits = (uint32_t)__shfl((int)my_word, j, 64);
    const int b = (int)(wj / A.W);
    const int e0 = (int)(wj - (int64_t)b * A.W) * 32;
    const int2* bm_row = A.bm_old + (int64_t)b * A.W;
    const float4* aq = A.a_q + (int64_t)b * A.ap4;
    const int32_t base = EMIT ? A.word_ptr[wj] : 0;
    const int32_t lim = EMIT ? A.word_ptr[wj + 1] : 0;   // (the count pass's total for this word: never written past)
    int32_t cnt = 0;                                   // kept edges of this word so far (uniform)
    int wlo = 0, whi = 0;
    if constexpr (WINDOW) { wlo = A.win_lo[b]; whi = A.win_hi[b]; }
    while (bits) {
      const int t = e0 + __ffs((int)bits) - 1;
      bits &= bits - 1u;
      const int beg = A.in_ptr[t], end = A.in_ptr[t + 1];
      for (int c0 = beg; c0 < end; c0 += 64) {
        const int c = c0 + lane;
        bool keep = false;
        int hd = 0, r = 0;
        float alpha = 0.f;
        if (c < end) {
          const int2 hr = A.in_hr[c];
          hd = hr.x; r = hr.y;
          const int2 wp = bm_row[hd >> 5];
          bool valid = rg::bm_has(wp, hd);
          if constexpr (WINDOW) {
            const int row = A.in_time[c];
            valid = valid && (row >= A.n_data || (row >= wlo && row < whi));
          }
          if (valid) {
            const int s = rg::bm_rank(wp, hd);
            float z = b_alpha;
            for (int k = 0; k < A.ap4; ++k) {
              const float4 as = A.a_s[(int64_t)s * A.ap4 + k];
              const float4 ar = A.a_r[(int64_t)r * A.ap4 + k];
              rg::attn_acc_fwd(z, rg::attn_w4(A.w_alpha, A.attn_dim, k), as, ar, aq[k]);
            }
            alpha = rg::attn_alpha(z);
            keep = alpha >= A.tau;
          }
        }
        const unsigned long long m = __ballot(keep);
        if (keep) {
          if constexpr (EMIT) {
            const int32_t idx = base + cnt + __popcll(m & ((1ull << lane) - 1ull));
            if (idx < lim) {
              A.edges[idx] = make_int4(b, hd, r, t);
              A.alpha[idx] = alpha;
              if constexpr (TIME) A.time_out[idx] = A.in_time[c];
            }
          } else {
            atomicOr(&A.marks_prev[(int64_t)b * A.W + (hd >> 5)], 1u << (hd & 31));   // result unused: non-returning
          }
        }
        cnt += __popcll(m);
      }
    }
    if (lane == j) my_count = cnt;
  }
  if constexpr (!EMIT) {
    if (wi < A.n_words) A.word_count[wi] = my_count;
  }
}

__global__ void gather_kernel(int64_t n, int hop, const int4* __restrict__ edges, const float* __restrict__ alpha,
                              const int64_t* __restrict__ row_first, const int64_t* __restrict__ row_base, int B, int64_t n_out,
                              int32_t* __restrict__ out_edges, float* __restrict__ out_alpha) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int4 e = edges[i];
  if (e.x < 0 || e.x >= B) return;
  const int64_t dst = row_base[e.x] + (i - row_first[e.x]);
  if (dst < 0 || dst >= n_out) return;
  int32_t* o = out_edges + dst * 5;
  o[0] = e.x; o[1] = hop; o[2] = e.y; o[3] = e.z; o[4] = e.w;
  out_alpha[dst] = alpha[i];
}

// checks shared by the per-hop entry points
enum Setting { STATIC, TEMPORAL, WINDOWED };

int check_hop(const char* who, Setting setting, const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level) {
  RG_CHECK(level >= 1 && level < RG_MAX_LEVELS, "%s: level %d not in 1..%d", who, level, RG_MAX_LEVELS - 1);
  RG_CHECK(batch > 0 && n_ent > 0, "%s: batch=%d n_ent=%d must be positive", who, batch, n_ent);
  RG_CHECK(f != nullptr && g != nullptr, "%s: NULL frontier or graph", who);
  RG_CHECK(batch == f->B && n_ent == f->n_ent, "%s: batch=%d n_ent=%d but the frontier has batch %d, n_ent %d", who, batch, n_ent,
           f->B, f->n_ent);
  RG_CHECK(g->n_ent == f->n_ent, "%s: graph has %d entities, frontier %d", who, g->n_ent, f->n_ent);
  if (setting == WINDOWED) {
    RG_CHECK(g->n_time > 0 && g->in_time, "%s: the graph has no row ids (build it with rg_tgraph_create, time field = data row)", who);
    RG_CHECK(f->win_lo && f->win_hi, "%s: call rg_frontier_set_window first", who);
  } else if (setting == TEMPORAL) {
    RG_CHECK(g->n_time > 0 && g->in_time, "%s: temporal graphs only (rg_tgraph_create)", who);
    RG_CHECK(f->win_lo == nullptr, "%s: the frontier has a window set (use rg_xexplain_count / rg_xexplain_emit)", who);
  } else {
    RG_CHECK(g->n_time == 0, "%s: static graphs only (rg_graph_create)", who);
  }
  RG_CHECK(level <= f->level && level > f->level - f->n_levels + 1, "%s: level %d not resident (current %d, %d kept)", who, level,
           f->level, f->n_levels);
  return 0;
}

int fill_args(const char* who, const rg_frontier* f, const rg_graph* g, int32_t level, const uint32_t* marks, const float* a_s,
              const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha, int32_t attn_dim,
              float min_alpha, ExArgs* A) {
  RG_CHECK(marks && a_s && a_r && a_q && w_alpha && b_alpha, "%s: NULL argument", who);
  RG_CHECK(attn_dim > 0 && ap >= attn_dim && ap % 4 == 0 && ap <= 128, "%s: attn_dim=%d ap=%d", who, attn_dim, ap);
  RG_CHECK((((uintptr_t)a_s | (uintptr_t)a_r | (uintptr_t)a_q) & 15) == 0, "%s: attention tables must be 16-B aligned", who);
  RG_CHECK(min_alpha == min_alpha, "%s: min_alpha is NaN", who);
  A->marks = marks; A->n_words = (int64_t)f->B * f->W; A->W = f->W;
  A->in_ptr = g->in_ptr; A->in_hr = g->in_hr; A->bm_old = f->bm_of(level - 1);
  A->a_s = (const float4*)a_s; A->a_r = (const float4*)a_r; A->a_q = (const float4*)a_q; A->ap4 = ap / 4;
  A->w_alpha = w_alpha; A->b_alpha = b_alpha; A->attn_dim = attn_dim; A->tau = min_alpha;
  A->marks_prev = nullptr; A->word_count = nullptr; A->word_ptr = nullptr; A->edges = nullptr; A->alpha = nullptr;
  return 0;
}

size_t count_bytes(const rg_frontier* f) { return rg::align_up((size_t)f->B * f->W * 4, 256); }

// the extrapolation setting's part of the arguments: the frontier's windows and the graph's row ids
void fill_window(const rg_frontier* f, const rg_graph* g, XExArgs* A) {
  A->in_time = g->in_time; A->time_out = nullptr;
  A->win_lo = f->win_lo; A->win_hi = f->win_hi; A->n_data = f->win_n_data;
}

template <Setting SETTING>
int count_hop(const char* who, const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level,
              const uint32_t* marks, const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
              const float* b_alpha, int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
              size_t scratch_bytes, int64_t* n_edges_host, void* stream) {
  if (check_hop(who, SETTING, f, g, batch, n_ent, level)) return 1;
  std::conditional_t<SETTING == WINDOWED, XExArgs, ExArgs> A;     // (the temporal attention does not read the time: the static pass)
  if constexpr (SETTING == WINDOWED) fill_window(f, g, &A);
  if (fill_args(who, f, g, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, min_alpha, &A)) return 1;
  RG_CHECK(marks_prev_out && word_ptr_out && n_edges_host, "%s: NULL argument", who);
  RG_CHECK(scratch && scratch_bytes >= rg_explain_scratch_bytes(f) && ((uintptr_t)scratch & 255) == 0,      // (declared in redgnn.h)
           "%s: scratch %zu B < required %zu B (or not 256-B aligned)", who, scratch_bytes, rg_explain_scratch_bytes(f));
  hipStream_t s = (hipStream_t)stream;
  A.marks_prev = marks_prev_out;
  A.word_count = (int32_t*)scratch;
  if (rg::zero_async(marks_prev_out, (size_t)A.n_words * 4, s)) return 1;
  hipLaunchKernelGGL((explain_kernel<false, false, SETTING == WINDOWED>), dim3(rg::ceil_div(A.n_words, EX_BLOCK)), dim3(EX_BLOCK), 0, s, A);
  RG_LAUNCH_CHECK();
  int32_t* scan_scr = (int32_t*)((char*)scratch + count_bytes(f));
  if (rg::scan_exclusive((const uint32_t*)A.word_count, word_ptr_out, A.n_words, false, word_ptr_out + A.n_words, scan_scr, s)) return 1;
  int32_t total = 0;
  RG_HIP(hipMemcpyAsync(&total, word_ptr_out + A.n_words, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  RG_HIP(hipStreamSynchronize(s));
  *n_edges_host = total;
  return 0;
}

template <bool TIME, bool WINDOW = false>
int emit_hop(const char* who, const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
             const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
             int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out, int32_t* time_out,
             void* stream) {
  if (check_hop(who, WINDOW ? WINDOWED : TIME ? TEMPORAL : STATIC, f, g, batch, n_ent, level)) return 1;
  std::conditional_t<WINDOW, XExArgs, std::conditional_t<TIME, TExArgs, ExArgs>> A;
  if constexpr (WINDOW) fill_window(f, g, &A);
  if (fill_args(who, f, g, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, min_alpha, &A)) return 1;
  RG_CHECK(word_ptr && edges_out && alpha_out && (!TIME || time_out), "%s: NULL argument", who);
  RG_CHECK(((uintptr_t)edges_out & 15) == 0, "%s: edges_out must be 16-B aligned", who);
  A.word_ptr = word_ptr; A.edges = (int4*)edges_out; A.alpha = alpha_out;
  if constexpr (TIME) { A.in_time = g->in_time; A.time_out = time_out; }
  hipLaunchKernelGGL((explain_kernel<true, TIME, WINDOW>), dim3(rg::ceil_div(A.n_words, EX_BLOCK)), dim3(EX_BLOCK), 0, (hipStream_t)stream, A);
  RG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

size_t rg_explain_scratch_bytes(const rg_frontier* f) {
  if (!f) return 0;
  return count_bytes(f) + rg::scan_scratch_elems((int64_t)f->B * f->W) * 4 + 256;
}

int rg_explain_seed(const rg_frontier* f, int32_t batch, int32_t n_ent, int32_t level, const int32_t* objs, uint32_t* marks_out,
                    uint8_t* reached_out, void* stream) {
  RG_CHECK(level >= 1 && level < RG_MAX_LEVELS, "rg_explain_seed: level %d not in 1..%d", level, RG_MAX_LEVELS - 1);
  RG_CHECK(batch > 0 && n_ent > 0, "rg_explain_seed: batch=%d n_ent=%d must be positive", batch, n_ent);
  RG_CHECK(f != nullptr, "rg_explain_seed: NULL frontier");
  RG_CHECK(objs && marks_out && reached_out, "rg_explain_seed: NULL argument");
  RG_CHECK(batch == f->B && n_ent == f->n_ent, "rg_explain_seed: batch=%d n_ent=%d but the frontier has batch %d, n_ent %d", batch,
           n_ent, f->B, f->n_ent);
  RG_CHECK(level <= f->level && level > f->level - f->n_levels, "rg_explain_seed: level %d not resident (current %d, %d kept)", level,
           f->level, f->n_levels);
  hipStream_t s = (hipStream_t)stream;
  if (rg::zero_async(marks_out, (size_t)f->B * f->W * 4, s)) return 1;
  hipLaunchKernelGGL(seed_kernel, dim3(rg::ceil_div(f->B, 256)), dim3(256), 0, s, f->bm_of(level), f->B, f->W, f->n_ent, objs,
                     marks_out, reached_out);
  RG_LAUNCH_CHECK();
  return 0;
}

int rg_explain_count(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                     int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
                     size_t scratch_bytes, int64_t* n_edges_host, void* stream) {
  return count_hop<STATIC>("rg_explain_count", f, g, batch, n_ent, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, min_alpha,
                   marks_prev_out, word_ptr_out, scratch, scratch_bytes, n_edges_host, stream);
}

int rg_texplain_count(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                      const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                      int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
                      size_t scratch_bytes, int64_t* n_edges_host, void* stream) {
  return count_hop<TEMPORAL>("rg_texplain_count", f, g, batch, n_ent, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, min_alpha,
                   marks_prev_out, word_ptr_out, scratch, scratch_bytes, n_edges_host, stream);
}

int rg_explain_emit(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                    const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                    int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out, void* stream) {
  return emit_hop<false>("rg_explain_emit", f, g, batch, n_ent, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, min_alpha,
                         word_ptr, edges_out, alpha_out, nullptr, stream);
}

int rg_texplain_emit(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                     int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out,
                     int32_t* time_out, void* stream) {
  return emit_hop<true>("rg_texplain_emit", f, g, batch, n_ent, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, min_alpha,
                        word_ptr, edges_out, alpha_out, time_out, stream);
}

int rg_xexplain_count(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                      const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                      int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
                      size_t scratch_bytes, int64_t* n_edges_host, void* stream) {
  return count_hop<WINDOWED>("rg_xexplain_count", f, g, batch, n_ent, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim,
                   min_alpha, marks_prev_out, word_ptr_out, scratch, scratch_bytes, n_edges_host, stream);
}

int rg_xexplain_emit(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                     int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out,
                     int32_t* row_out, void* stream) {
  return emit_hop<true, true>("rg_xexplain_emit", f, g, batch, n_ent, level, marks, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim,
                              min_alpha, word_ptr, edges_out, alpha_out, row_out, stream);
}

int rg_explain_gather(int64_t n, int32_t hop, int32_t batch, const int32_t* edges, const float* alpha, const int64_t* row_first,
                      const int64_t* row_base, int64_t n_out, int32_t* edges_out, float* alpha_out, void* stream) {
  RG_CHECK(n >= 0 && n_out >= 0 && batch > 0 && hop >= 1, "rg_explain_gather: n=%lld n_out=%lld batch=%d hop=%d", (long long)n,
           (long long)n_out, batch, hop);
  if (n == 0) return 0;
  RG_CHECK(edges && alpha && row_first && row_base && edges_out && alpha_out, "rg_explain_gather: NULL argument");
  RG_CHECK(((uintptr_t)edges & 15) == 0, "rg_explain_gather: edges must be 16-B aligned");
  hipLaunchKernelGGL(gather_kernel, dim3(rg::ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, n, hop, (const int4*)edges, alpha,
                     row_first, row_base, batch, n_out, edges_out, alpha_out);
  RG_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
