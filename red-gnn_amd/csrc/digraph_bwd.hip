// The adjoint of one rg_digraph_layer_fwd hop (static form) with respect to a gate on every edge, the source states and their
// attention projection (rg_digraph_layer_bwd): the executor behind explain.RDigraph.saliency.  With a gate g_e multiplying the
// message of edge e, agg[o] = sum_e g_e alpha_e (hidden[s] + rela[r]), and G = grad_agg, per edge e = (s, r, o), b = row_of_dst[o]:
//
//   alpha_e = sigmoid(w . relu((a_s[s] + a_r[r]) + a_q[b]) + b_alpha)        attn.h attn_acc_fwd / attn_alpha: the forward's float
//   g_alpha = <G[o], hidden[s] + rela[r]>
//   grad_gate[e]     = alpha_e * g_alpha                                      (at g == 1)
//   grad_hidden[s]  += alpha_e * G[o]
//   g_p              = g_alpha * alpha_e * (1 - alpha_e)
//   grad_a_s[s]     += g_p * w * 1[(a_s[s] + a_r[r]) + a_q[b] > 0]
//
// rela, a_r, a_q, w_alpha and b_alpha are constants here: there are no parameter gradients.
//
// The sums run over a SOURCE's out-edges, so the hop comes with a source-segmented view next to the destination-ordered lists the
// forward takes: src_ptr [n_src + 1] over the positions k of edge_of [E], edge_of[k] = e the edge's position in the destination-ordered
// list (a stable permutation: a source's edges in list order), dst_of_edge[e] = o.
//
// Mapping (wave64), the forward's with source and destination exchanged: a source is owned by a group of G lanes, G * 4 >= ld floats,
// one float4 of its row per lane, 64 / G sources per wave.  A round takes G of the source's edges: lane j forms the attention scalar of
// edge j and the sign bits of its pre-activation, then the group walks the round's edges in order, each lane gathering its float4 of
// G[o] and rela[r], four edges' gathers in flight; the row dot product is reduced inside the group and lane j keeps edge j's.  Lane j
// then stores grad_gate of its edge and adds its edge's g_p * 1[pre > 0] to its own attention accumulator; the lanes' accumulators
// are added across the group once, when the item ends, and the total is multiplied by w there (w is constant over the sum).  All
// lanes of a wave run the same number of rounds (the longest source's) with their stores predicated, so the lane exchanges never
// read an inactive lane.
//
// Split rule, the forward's: a source of more than DIGRAPH_CHUNK out-edges is cut into chunks counted from ITS OWN first edge; every
// chunk is an item of the same launch that sums into partial rows, and a second launch adds the partial rows in chunk order.  Hop 1 of
// an r-digraph is the case: a row's only source is its subject, with every hop-1 edge.  No float atomics: the sums of a source are
// formed in list order inside a chunk and in chunk order across chunks, so every output has the same bits on every run and does not
// depend on what else the call carries.
//
// The timed form (rg_digraph_tlayer_bwd, template parameter TIMED; the static instantiation compiles to what it did without it), the
// adjoint of rg_digraph_tlayer_fwd: the message is hidden[hrow] + (rela[rrow] + time_tab[trow]) with the rows digraph_fwd_kernel<...,
// TIMED> forms (64-bit differences, |dt| clamped to n_time - 1, the n_dir = 1 lag clamped to 0 .. n_time - 1), alpha_e read from the
// un-directed s and r.  The work item is a DIRECTED source row u - u = 3 s + dir for n_dir = 3, u = s for n_dir = 1 - and the
// source-segmented view is sorted, stably, by u: src_ptr [n_dir * n_src + 1].  An item then loads one state row, hidden[u], and one
// attention row, a_s[u / n_dir], and keeps one acc_h as the static kernel does; a source whose edges span three directions is three
// items, and grad_a_s_dir [n_dir * n_src, ap] has a row per item (the caller adds a source's three).  The edge's direction is formed
// again per edge for rrow and trow (it is not taken from u, so an inconsistent view reads other rows, never out of bounds); the time
// table's gather is the only added traffic.  The split rule counts chunks per directed row.
//
// The gated, replicated form (rg_digraph_layer_bwd_gated, template parameter GATED; static only, and the other instantiations compile
// to what they did without it), the adjoint of rg_digraph_layer_fwd_gated at the gates g = fmaf(t[k], gate_hi[e] - gate_lo[e],
// gate_lo[e]): n_rep replicas, replica k with its own hidden, a_s and grad_agg rows (k * n_src + s, k * n_dst + o) and its own outputs
// (grad_gate[k * E + e], state rows k * n_src + s, partial rows k * n_chunks + slot); the source view, rel, row_of_dst, rela, a_r, a_q
// and w are shared.  With c = g * alpha_e (rounded once, the forward's coefficient):
//       grad_gate[e]     = alpha_e * g_alpha                   the derivative with respect to g itself: the gate does not scale it
//       grad_hidden[s]  += c * G[o]
//       grad_a_s[s]     += g * (g_alpha * alpha_e * (1 - alpha_e)) * w * 1[pre > 0]
// so that g == 1 leaves the ungated kernel's bits.  An item is a (replica, source or chunk) pair, item k * n_items + i: a group works
// exactly as it does in an n_rep = 1 call.  The combine launch has a grid row per replica.
//
// A gate per (replica, edge) (rg_digraph_layer_bwd_gates): the replica stride on the gate pointers that digraph_fwd.hip describes.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "attn.h"

namespace rgdb {
namespace {

constexpr int DIGRAPH_CHUNK = RG_DIGRAPH_CHUNK;   // edges per chunk of a cut source (include/redgnn.h)
constexpr int DB_BLOCK = 256;                     // 4 waves

struct DbArgs {
  int n_src, n_items;          // items: [0, n_src) the sources themselves, then the chunks of the cut ones
  int E, n_dst, n_rela_rows, B;
  const int32_t* src_ptr;
  const int32_t* edge_of;
  const int32_t* dst_of_edge;
  const int32_t* rel;
  const int32_t* row_of_dst;
  const int4* chunks;          // [n_items - n_src] {source, first position, end, slot of the partial rows}
  const float4* hidden;
  const float4* rela;
  const float4* grad_agg;
  int ld4;
  const float4* a_s;
  const float4* a_r;
  const float4* a_q;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  float* grad_gate;
  float4* grad_hidden;         // nullptr: not wanted (then neither is grad_a_s)
  float4* grad_a_s;
  float4* partial_h;           // [n_chunks, ld4]
  float4* partial_as;          // [n_chunks, AP4]
};

// what the timed form (rg_digraph_tlayer_bwd) reads on top: kept apart so that the static kernel's arguments stay what they were.  There
// n_src counts the DIRECTED source rows (the rows of hidden and of both state outputs).
struct DbTimedArgs : DbArgs {
  const int32_t* edge_time;    // [E], in the order of the destination-ordered list
  const int32_t* q_time;       // [B]
  const float4* time_tab;      // [n_dir * n_time, ld]
  int n_time, n_dir;           // n_dir 3: interpolation (rows by direction), 1: extrapolation form (one table of lags)
};

// what the gated form (rg_digraph_layer_bwd_gated) reads on top
struct DbGatedArgs : DbArgs {
  int n_rep, n_chunks;         // replicas; chunks of ONE replica (replica k's partial rows start at k * n_chunks)
  const float* t;              // [n_rep], or nullptr: 1 (the per-replica form)
  const float* gate_lo;        // [E] by position in the destination-ordered list, or nullptr: 0
  const float* gate_hi;        // [E], or nullptr: 1
  int gate_rep;                // replica k's gates start k * gate_rep floats further on (n_rep * E fits int32): 0, the shared pair, or
                               // E with gate_lo == gate_hi (rg_digraph_layer_bwd_gates)
};

template <bool TIMED, bool GATED>
using DbArgsOf = std::conditional_t<GATED, DbGatedArgs, std::conditional_t<TIMED, DbTimedArgs, DbArgs>>;

__device__ __forceinline__ int clampi(int x, int hi) { return min(max(x, 0), hi); }

template <int G, int AP4, bool TIMED, bool GATED>
__global__ __launch_bounds__(DB_BLOCK) void digraph_bwd_kernel(DbArgsOf<TIMED, GATED> A) {
  static_assert(!(TIMED && GATED), "the gated form is static");
  constexpr int PER_WAVE = 64 / G;
  const int lane = threadIdx.x & 63;
  const int lane_g = lane & (G - 1), gbase = lane & ~(G - 1);
  const int wave = blockIdx.x * (DB_BLOCK / 64) + (threadIdx.x >> 6);
  int item = wave * PER_WAVE + lane / G;
  int rep = 0;                                           // GATED: the item's replica, and the item inside it
  if constexpr (GATED) {
    rep = item / A.n_items;
    item -= rep * A.n_items;
    if (rep >= A.n_rep) { rep = 0; item = A.n_items; }   // past the last replica: no work
  }
  const bool row_lane = lane_g < A.ld4;
  const int lane_c = row_lane ? lane_g : A.ld4 - 1;      // loads never branch: idle lanes re-read the last float4

  // the item's source, range of positions and output rows; an item without work keeps beg == end and stores nothing
  int s = 0, beg = 0, end = 0;
  float4* out_h = nullptr;
  float4* out_as = nullptr;
  if (item < A.n_src) {
    s = item;
    const int lo = clampi(A.src_ptr[s], A.E), hi = clampi(A.src_ptr[s + 1], A.E);
    if (hi - lo <= DIGRAPH_CHUNK) {                      // (a cut source is written by the combine pass)
      beg = lo; end = max(hi, lo);
      if (A.grad_hidden) { out_h = A.grad_hidden + (int64_t)s * A.ld4; out_as = A.grad_a_s + (int64_t)s * AP4; }
      if constexpr (GATED)
        if (A.grad_hidden) { out_h += (int64_t)rep * A.n_src * A.ld4; out_as += (int64_t)rep * A.n_src * AP4; }
    }
  } else if (item < A.n_items) {
    const int4 c = A.chunks[item - A.n_src];
    s = clampi(c.x, A.n_src - 1);
    beg = clampi(c.y, A.E); end = min(max(clampi(c.z, A.E), beg), beg + DIGRAPH_CHUNK);
    if (A.grad_hidden) { out_h = A.partial_h + (int64_t)c.w * A.ld4; out_as = A.partial_as + (int64_t)c.w * AP4; }
    if constexpr (GATED)
      if (A.grad_hidden) { out_h += (int64_t)rep * A.n_chunks * A.ld4; out_as += (int64_t)rep * A.n_chunks * AP4; }
  }
  const float b_alpha = A.b_alpha[0];
  // GATED: the replica's rows of hidden, a_s and grad_agg, its grad_gate and its t
  int64_t srow = s;
  const float4* grad_agg = A.grad_agg;
  float* grad_gate = A.grad_gate;
  float t_rep = 1.f;
  if constexpr (GATED) {
    srow += (int64_t)rep * A.n_src;
    grad_agg += (int64_t)rep * A.n_dst * A.ld4;
    grad_gate += (int64_t)rep * A.E;
    if (A.t) t_rep = A.t[rep];
  }
  int gate_at = 0;                                       // GATED: where the replica's gates start (n_rep * E fits int32)
  if constexpr (GATED) gate_at = rep * A.gate_rep;
  const float4 hv = A.hidden[srow * A.ld4 + lane_c];
  const float4* as_p;
  if constexpr (TIMED) as_p = A.a_s + (int64_t)(s / A.n_dir) * AP4;      // the attention reads the un-directed source
  else as_p = A.a_s + srow * AP4;

  float4 acc_h = rg::f4zero();
  float4 acc_as[AP4];
#pragma unroll
  for (int k = 0; k < AP4; ++k) acc_as[k] = rg::f4zero();
  for (int c0 = beg; __any(c0 < end); c0 += G) {
    // ---- one edge per lane: indices, the attention scalar and the sign bits of its pre-activation ---------------
    const int c = c0 + lane_g;
    const bool valid = c < end;
    int e = 0, o = 0, r = 0, trow = 0;
    unsigned pos = 0;                                    // bit 4k + u: component 4k + u of (a_s + a_r) + a_q is > 0
    float alpha = 0.f, gate = 1.f, coef = 0.f;           // GATED: the edge's gate g and the message's coefficient c = g * alpha
    if (valid) {
      e = clampi(A.edge_of[c], A.E - 1);
      o = clampi(A.dst_of_edge[e], A.n_dst - 1);
      r = clampi(A.rel[e], A.n_rela_rows - 1);
      const int b = clampi(A.row_of_dst[o], A.B - 1);
      const float4* aq_p = A.a_q + (int64_t)b * AP4;
      float z = b_alpha;
      // (the timed form holds five more pointers and sizes in scalar registers: unrolled four times it would spill them at AP4 = 4)
#pragma clang loop unroll_count(AP4 >= (TIMED ? 4 : 8) ? 2 : AP4)
      for (int k = 0; k < AP4; ++k) {
        const float4 as = as_p[k], ar = A.a_r[(int64_t)r * AP4 + k], aq = aq_p[k];
        rg::attn_acc_fwd(z, rg::attn_w4(A.w_alpha, A.attn_dim, k), as, ar, aq);
        pos |= (unsigned)(as.x + ar.x + aq.x > 0.f) << (4 * k) | (unsigned)(as.y + ar.y + aq.y > 0.f) << (4 * k + 1) |
               (unsigned)(as.z + ar.z + aq.z > 0.f) << (4 * k + 2) | (unsigned)(as.w + ar.w + aq.w > 0.f) << (4 * k + 3);
      }
      alpha = rg::attn_alpha(z);
      if constexpr (GATED) {
        const float lo = A.gate_lo ? A.gate_lo[gate_at + e] : 0.f, hi = A.gate_hi ? A.gate_hi[gate_at + e] : 1.f;
        gate = fmaf(t_rep, hi - lo, lo);
        coef = gate * alpha;
      }
      if constexpr (TIMED) {
        // the rows of the message, as digraph_fwd_kernel forms them (the attention above read the un-directed r); 64-bit
        // differences, so that no pair of times overflows, and the time row clamped into its table
        const int64_t et = A.edge_time[e], qt = A.q_time[b];
        if (A.n_dir == 3) {
          const int64_t dt = et - qt;
          const int dir = dt > 0 ? 2 : (dt == 0 ? 1 : 0);
          r = dir * A.n_rela_rows + r;
          trow = dir * A.n_time + (int)min(dt < 0 ? -dt : dt, (int64_t)(A.n_time - 1));
        } else {
          trow = (int)min(max(qt - et, (int64_t)0), (int64_t)(A.n_time - 1));
        }
      }
    }
    const int cnt = min(max(end - c0, 0), G);
    // ---- the round's edges in order, every lane its float4 of the rows; four edges' gathers in flight -----------
    float g_alpha = 0.f;
    for (int j = 0; __any(j < cnt); j += 4) {
      int ou[4], ru[4], tu[4];
      float al[4];
      float4 gv[4], rv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // (slots past cnt hold o = r = 0: row 0 is read and not used)
        const int from = gbase + ((j + u) & (G - 1));
        ou[u] = __shfl(o, from, 64);
        ru[u] = __shfl(r, from, 64);
        al[u] = __shfl(GATED ? coef : alpha, from, 64);
        if constexpr (TIMED) tu[u] = __shfl(trow, from, 64);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) gv[u] = grad_agg[(int64_t)ou[u] * A.ld4 + lane_c];
#pragma unroll
      for (int u = 0; u < 4; ++u) rv[u] = A.rela[(int64_t)ru[u] * A.ld4 + lane_c];
      if constexpr (TIMED) {             // rela[rrow] + time_tab[trow] first, then hidden: the forward's association
        float4 tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tv[u] = A.time_tab[(int64_t)tu[u] * A.ld4 + lane_c];
#pragma unroll
        for (int u = 0; u < 4; ++u) { rv[u].x += tv[u].x; rv[u].y += tv[u].y; rv[u].z += tv[u].z; rv[u].w += tv[u].w; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        float p = gv[u].x * (hv.x + rv[u].x);
        p = fmaf(gv[u].y, hv.y + rv[u].y, p);
        p = fmaf(gv[u].z, hv.z + rv[u].z, p);
        p = fmaf(gv[u].w, hv.w + rv[u].w, p);
        const float dot = rg::group_sum<G>(row_lane ? p : 0.f);
        if (j + u < cnt) {
          acc_h.x = fmaf(al[u], gv[u].x, acc_h.x);
          acc_h.y = fmaf(al[u], gv[u].y, acc_h.y);
          acc_h.z = fmaf(al[u], gv[u].z, acc_h.z);
          acc_h.w = fmaf(al[u], gv[u].w, acc_h.w);
        }
        if (lane_g == j + u) g_alpha = dot;
      }
    }
    // ---- back on the edge's own lane: its gate gradient, and its share of the source's attention gradient ---------
    if (valid) {
      grad_gate[e] = alpha * g_alpha;
      float g_p = g_alpha * alpha * (1.f - alpha);
      if constexpr (GATED) g_p = gate * g_p;
#pragma unroll
      for (int k = 0; k < AP4; ++k) {      // (w is constant over the sum: it multiplies the total, below)
        acc_as[k].x += (pos >> (4 * k) & 1u) ? g_p : 0.f;
        acc_as[k].y += (pos >> (4 * k + 1) & 1u) ? g_p : 0.f;
        acc_as[k].z += (pos >> (4 * k + 2) & 1u) ? g_p : 0.f;
        acc_as[k].w += (pos >> (4 * k + 3) & 1u) ? g_p : 0.f;
      }
    }
  }
  if (out_h && row_lane) out_h[lane_g] = acc_h;
  // the lanes' attention accumulators added across the group (every lane of the wave takes part); float4 k stored by lane k mod G
#pragma unroll
  for (int k = 0; k < AP4; ++k) {
    const float4 w = rg::attn_w4(A.w_alpha, A.attn_dim, k);
    float4 t;
    t.x = w.x * rg::group_sum<G>(acc_as[k].x);
    t.y = w.y * rg::group_sum<G>(acc_as[k].y);
    t.z = w.z * rg::group_sum<G>(acc_as[k].z);
    t.w = w.w * rg::group_sum<G>(acc_as[k].w);
    if (out_as && lane_g == (k & (G - 1))) out_as[k] = t;
  }
}

// grad_hidden[s] and grad_a_s[s] of the cut sources: their chunks' partial rows added in chunk order, the first one initialising the
// sum.  A thread per float4: the ld4 of the state row, then the ap4 of the attention row.
// (gated form: grid row k is replica k, its partial rows n_chunks and its output rows n_src further on)
__global__ void digraph_bwd_combine_kernel(const int4* __restrict__ hubs, int n_hubs, const float4* __restrict__ partial_h,
                                           const float4* __restrict__ partial_as, float4* __restrict__ grad_hidden,
                                           float4* __restrict__ grad_a_s, int ld4, int ap4, int64_t n_chunks, int64_t n_src) {
  partial_h += blockIdx.y * n_chunks * ld4;
  partial_as += blockIdx.y * n_chunks * ap4;
  grad_hidden += blockIdx.y * n_src * ld4;
  grad_a_s += blockIdx.y * n_src * ap4;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int w = ld4 + ap4;
  const int64_t h = tid / w;
  int c = (int)(tid - h * w);
  if (h >= n_hubs) return;
  const int4 hub = hubs[h];                              // {source, first slot, chunks, -}
  const bool state = c < ld4;
  const int stride = state ? ld4 : ap4;
  if (!state) c -= ld4;
  const float4* p = (state ? partial_h : partial_as) + (int64_t)hub.y * stride + c;
  float4 acc = p[0];
  for (int k = 1; k < hub.z; ++k) {
    const float4 v = p[(int64_t)k * stride];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  (state ? grad_hidden : grad_a_s)[(int64_t)hub.x * stride + c] = acc;
}

// the cut sources of a CSR on the host: how many, and how many chunks they make
void count_cuts(const int32_t* ptr, int32_t n_src, int64_t* n_hubs, int64_t* n_chunks) {
  *n_hubs = *n_chunks = 0;
  for (int32_t s = 0; s < n_src; ++s) {
    const int64_t len = (int64_t)ptr[s + 1] - ptr[s];
    if (len > DIGRAPH_CHUNK) { ++*n_hubs; *n_chunks += rg::ceil_div(len, DIGRAPH_CHUNK); }
  }
}

size_t list_bytes(int64_t n_hubs, int64_t n_chunks) { return rg::align_up((size_t)(n_hubs + n_chunks) * sizeof(int4), 256); }
size_t rows_bytes(int64_t n_chunks, int32_t width) { return rg::align_up((size_t)n_chunks * width * sizeof(float), 256); }

template <int G, int AP4, bool TIMED, bool GATED = false>
int launch(const DbArgsOf<TIMED, GATED>& A, hipStream_t s) {
  int64_t items = A.n_items;
  if constexpr (GATED) items *= A.n_rep;
  const int64_t waves = rg::ceil_div(items, 64 / G);
  hipLaunchKernelGGL((digraph_bwd_kernel<G, AP4, TIMED, GATED>), dim3((unsigned)rg::ceil_div(waves, DB_BLOCK / 64)), dim3(DB_BLOCK), 0, s, A);
  RG_LAUNCH_CHECK();
  return 0;
}

// the time arguments of rg_digraph_tlayer_bwd; nullptr: the static entry point
struct TimeIn {
  const int32_t* edge_time;
  const int32_t* q_time;
  const float* time_tab;
  int32_t n_time, n_dir;
};

// the gate arguments of rg_digraph_layer_bwd_gated / _gates; nullptr: the ungated entry points.  per_rep (rg_digraph_layer_bwd_gates):
// gate_lo == gate_hi is the [n_rep, E] array and t is not read, as in digraph_fwd.hip
struct GateIn {
  int32_t n_rep;
  const float* t;
  const float* gate_lo;
  const float* gate_hi;
  bool per_rep;
};

size_t scratch_need(int64_t n_hubs, int64_t n_chunks, int32_t ld, int32_t ap, int64_t n_rep) {
  return n_hubs ? list_bytes(n_hubs, n_chunks) + rows_bytes(n_rep * n_chunks, ld) + rows_bytes(n_rep * n_chunks, ap) : 0;
}

// every entry point: every check, then the chunk list, the layer launch and the combine launch.  n_rows: the rows of the source view,
// of hidden and of the state outputs - n_src, or n_dir * n_src directed rows in the timed form.
int run(const char* who, const TimeIn* T, const GateIn* Q, int32_t n_src, int32_t n_dst, int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host,
        const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel, const int32_t* row_of_dst, int32_t n_rela_rows,
        int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q,
        int32_t ap, const float* w_alpha, const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_gate,
        float* grad_hidden, float* grad_a_s, void* scratch, size_t scratch_bytes, void* stream) {
  RG_CHECK(n_src >= 0 && n_dst >= 0 && n_edges >= 0 && n_edges < ((int64_t)1 << 31),
           "%s: n_src=%d n_dst=%d n_edges=%lld (need 0 <= n_src, 0 <= n_dst, 0 <= n_edges < 2^31)", who, n_src, n_dst, (long long)n_edges);
  RG_CHECK(n_rela_rows >= 0 && batch >= 0, "%s: n_rela_rows=%d batch=%d (negative size)", who, n_rela_rows, batch);
  RG_CHECK(d > 0 && ld >= d && ld % 4 == 0 && ld <= 256, "%s: d=%d ld=%d (need ld%%4==0, d<=ld<=256)", who, d, ld);
  RG_CHECK(attn_dim > 0 && ap >= attn_dim && ap % 4 == 0, "%s: attn_dim=%d ap=%d", who, attn_dim, ap);
  if (T) {
    RG_CHECK(T->n_dir == 1 || T->n_dir == 3, "%s: n_dir=%d (need 1 or 3)", who, T->n_dir);
    RG_CHECK(T->n_time > 0 && (int64_t)T->n_dir * T->n_time < ((int64_t)1 << 31), "%s: n_time=%d (need a positive table size)", who,
             T->n_time);
    RG_CHECK((int64_t)3 * n_src < ((int64_t)1 << 31) && (int64_t)3 * n_rela_rows < ((int64_t)1 << 31),
             "%s: n_src=%d n_rela_rows=%d (three rows each overflow int32)", who, n_src, n_rela_rows);
  }
  const int64_t n_rep = Q ? Q->n_rep : 1;
  if (Q) {
    RG_CHECK(!T, "%s: the gated form is static", who);
    RG_CHECK(n_rep >= 1, "%s: n_rep=%lld (need at least one replica)", who, (long long)n_rep);
    RG_CHECK(n_rep * std::max(n_src, n_dst) < ((int64_t)1 << 31) && n_rep * n_edges < ((int64_t)1 << 31),
             "%s: n_rep=%lld times n_src=%d, n_dst=%d or n_edges=%lld overflows int32", who, (long long)n_rep, n_src, n_dst,
             (long long)n_edges);
    if (Q->per_rep) RG_CHECK(Q->gate_lo, "%s: NULL argument (gate)", who);
    else RG_CHECK(Q->t, "%s: NULL argument (t)", who);
    RG_CHECK(n_rep <= 65535, "%s: n_rep=%lld (at most 65535: the combine launch has a grid row per replica)", who, (long long)n_rep);
  }
  RG_CHECK((grad_hidden == nullptr) == (grad_a_s == nullptr), "%s: grad_hidden and grad_a_s come together or not at all", who);
  if (n_src == 0) {
    RG_CHECK(n_edges == 0, "%s: %lld edges without a source", who, (long long)n_edges);
    return 0;
  }
  const int32_t n_rows = T ? T->n_dir * n_src : n_src;
  RG_CHECK(src_ptr_host, "%s: NULL argument (src_ptr_host)", who);
  RG_CHECK(src_ptr_host[0] == 0, "%s: src_ptr starts at %d, not 0", who, src_ptr_host[0]);
  for (int32_t s = 0; s < n_rows; ++s)
    RG_CHECK(src_ptr_host[s + 1] >= src_ptr_host[s], "%s: src_ptr decreases at source %d", who, s);
  RG_CHECK(src_ptr_host[n_rows] == n_edges, "%s: src_ptr ends at %d, not at the number of edges %lld", who, src_ptr_host[n_rows],
           (long long)n_edges);
  if (n_edges == 0) return 0;                            // nothing to sum and nothing launched: the caller owns the outputs
  RG_CHECK(src_ptr && edge_of && dst_of_edge && rel && row_of_dst && hidden && rela && a_s && a_r && a_q && w_alpha && b_alpha &&
           grad_agg && grad_gate, "%s: NULL argument", who);
  RG_CHECK(!T || (T->edge_time && T->q_time && T->time_tab), "%s: NULL argument (edge_time, q_time or time_tab)", who);
  RG_CHECK(n_dst > 0 && n_rela_rows > 0 && batch > 0, "%s: edges but n_dst=%d n_rela_rows=%d batch=%d", who, n_dst, n_rela_rows, batch);
  RG_CHECK((((uintptr_t)hidden | (uintptr_t)rela | (uintptr_t)a_s | (uintptr_t)a_r | (uintptr_t)a_q | (uintptr_t)grad_agg |
             (uintptr_t)grad_hidden | (uintptr_t)grad_a_s | (uintptr_t)scratch | (uintptr_t)(T ? T->time_tab : nullptr)) & 15) == 0,
           "%s: float buffers must be 16-B aligned", who);
  int64_t n_hubs, n_chunks;
  count_cuts(src_ptr_host, n_rows, &n_hubs, &n_chunks);
  RG_CHECK(n_rep * ((int64_t)n_rows + n_chunks) < ((int64_t)1 << 31) - 64, "%s: %lld items overflow int32", who,
           (long long)(n_rep * (n_rows + n_chunks)));
  const size_t need = scratch_need(n_hubs, n_chunks, ld, ap, n_rep);
  RG_CHECK(need == 0 || (scratch && scratch_bytes >= need), "%s: scratch %zu B < required %zu B", who, scratch ? scratch_bytes : (size_t)0,
           need);

  DbTimedArgs A;
  A.n_src = n_rows; A.n_items = (int)(n_rows + n_chunks); A.E = (int)n_edges; A.n_dst = n_dst; A.n_rela_rows = n_rela_rows; A.B = batch;
  A.src_ptr = src_ptr; A.edge_of = edge_of; A.dst_of_edge = dst_of_edge; A.rel = rel; A.row_of_dst = row_of_dst;
  A.hidden = (const float4*)hidden; A.rela = (const float4*)rela; A.grad_agg = (const float4*)grad_agg; A.ld4 = ld / 4;
  A.a_s = (const float4*)a_s; A.a_r = (const float4*)a_r; A.a_q = (const float4*)a_q;
  A.w_alpha = w_alpha; A.b_alpha = b_alpha; A.attn_dim = attn_dim;
  A.grad_gate = grad_gate; A.grad_hidden = (float4*)grad_hidden; A.grad_a_s = (float4*)grad_a_s;
  A.edge_time = T ? T->edge_time : nullptr; A.q_time = T ? T->q_time : nullptr; A.time_tab = T ? (const float4*)T->time_tab : nullptr;
  A.n_time = T ? T->n_time : 0; A.n_dir = T ? T->n_dir : 0;
  int4* hubs_dev = (int4*)scratch;
  A.chunks = hubs_dev + n_hubs;
  A.partial_h = n_hubs ? (float4*)((char*)scratch + list_bytes(n_hubs, n_chunks)) : nullptr;
  A.partial_as = n_hubs ? (float4*)((char*)A.partial_h + rows_bytes(n_rep * n_chunks, ld)) : nullptr;
  // every argument error is out before anything is enqueued: the width dispatch is probed first
  if (rg::with_ap4(ap / 4, who, [](auto) { return 0; })) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (n_hubs) {
    std::vector<int4> list((size_t)(n_hubs + n_chunks));
    int64_t h = 0, slot = 0;
    for (int32_t v = 0; v < n_rows; ++v) {
      const int32_t lo = src_ptr_host[v], hi = src_ptr_host[v + 1];
      if (hi - lo <= DIGRAPH_CHUNK) continue;
      const int n_c = (int)rg::ceil_div(hi - lo, DIGRAPH_CHUNK);
      list[h++] = make_int4(v, (int)slot, n_c, 0);
      for (int k = 0; k < n_c; ++k, ++slot)
        list[n_hubs + slot] = make_int4(v, lo + k * DIGRAPH_CHUNK, std::min(hi, lo + (k + 1) * DIGRAPH_CHUNK), (int)slot);
    }
    // (a copy from pageable memory: the runtime is done with the vector when the call returns)
    RG_HIP(hipMemcpyAsync(hubs_dev, list.data(), list.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  }
  const int rc = rg::with_g(A.ld4, [&](auto g) {
    return rg::with_ap4(ap / 4, who, [&](auto a4) {
      if (T) return launch<decltype(g)::value, decltype(a4)::value, true>(A, s);
      if (Q) {
        DbGatedArgs GA;
        static_cast<DbArgs&>(GA) = A;
        GA.n_rep = (int)n_rep; GA.n_chunks = (int)n_chunks; GA.t = Q->t; GA.gate_lo = Q->gate_lo; GA.gate_hi = Q->gate_hi;
        GA.gate_rep = Q->per_rep ? (int)n_edges : 0;
        return launch<decltype(g)::value, decltype(a4)::value, false, true>(GA, s);
      }
      return launch<decltype(g)::value, decltype(a4)::value, false>(A, s);
    });
  });
  if (rc) return rc;
  if (n_hubs && grad_hidden) {
    const int64_t threads = n_hubs * (A.ld4 + ap / 4);
    hipLaunchKernelGGL(digraph_bwd_combine_kernel, dim3((unsigned)rg::ceil_div(threads, 256), (unsigned)n_rep), dim3(256), 0, s, hubs_dev,
                       (int)n_hubs, (const float4*)A.partial_h, (const float4*)A.partial_as, A.grad_hidden, A.grad_a_s, A.ld4, ap / 4,
                       n_chunks, (int64_t)n_rows);
    RG_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace rgdb

extern "C" size_t rg_digraph_layer_bwd_scratch_bytes(const int32_t* src_ptr_host, int32_t n_src, int32_t ld, int32_t ap) {
  if (!src_ptr_host || n_src <= 0 || ld <= 0 || ap <= 0) return 0;
  for (int32_t s = 0; s < n_src; ++s)
    if (src_ptr_host[s + 1] < src_ptr_host[s]) return 0;
  int64_t n_hubs, n_chunks;
  rgdb::count_cuts(src_ptr_host, n_src, &n_hubs, &n_chunks);
  if (n_hubs == 0) return 0;
  return rgdb::scratch_need(n_hubs, n_chunks, ld, ap, 1);
}

extern "C" size_t rg_digraph_layer_bwd_gated_scratch_bytes(const int32_t* src_ptr_host, int32_t n_src, int32_t ld, int32_t ap,
                                                           int32_t n_rep) {
  if (!src_ptr_host || n_src <= 0 || ld <= 0 || ap <= 0 || n_rep < 1) return 0;
  for (int32_t s = 0; s < n_src; ++s)
    if (src_ptr_host[s + 1] < src_ptr_host[s]) return 0;
  int64_t n_hubs, n_chunks;
  rgdb::count_cuts(src_ptr_host, n_src, &n_hubs, &n_chunks);
  return rgdb::scratch_need(n_hubs, n_chunks, ld, ap, n_rep);
}

extern "C" int rg_digraph_layer_bwd_gated(int32_t n_rep, const float* t, const float* gate_lo, const float* gate_hi, int32_t n_src,
                                          int32_t n_dst, int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host,
                                          const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel, const int32_t* row_of_dst,
                                          int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld,
                                          const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                                          const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_gate,
                                          float* grad_hidden, float* grad_a_s, void* scratch, size_t scratch_bytes, void* stream) {
  const rgdb::GateIn Q{n_rep, t, gate_lo, gate_hi, false};
  return rgdb::run("rg_digraph_layer_bwd_gated", nullptr, &Q, n_src, n_dst, n_edges, src_ptr, src_ptr_host, edge_of, dst_of_edge, rel,
                   row_of_dst, n_rela_rows, batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, grad_agg, grad_gate,
                   grad_hidden, grad_a_s, scratch, scratch_bytes, stream);
}

extern "C" int rg_digraph_layer_bwd_gates(int32_t n_rep, const float* gate, int32_t n_src, int32_t n_dst, int64_t n_edges,
                                          const int32_t* src_ptr, const int32_t* src_ptr_host, const int32_t* edge_of,
                                          const int32_t* dst_of_edge, const int32_t* rel, const int32_t* row_of_dst, int32_t n_rela_rows,
                                          int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld, const float* a_s,
                                          const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                                          int32_t attn_dim, const float* grad_agg, float* grad_gate, float* grad_hidden, float* grad_a_s,
                                          void* scratch, size_t scratch_bytes, void* stream) {
  const rgdb::GateIn Q{n_rep, nullptr, gate, gate, true};
  return rgdb::run("rg_digraph_layer_bwd_gates", nullptr, &Q, n_src, n_dst, n_edges, src_ptr, src_ptr_host, edge_of, dst_of_edge, rel,
                   row_of_dst, n_rela_rows, batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, grad_agg, grad_gate,
                   grad_hidden, grad_a_s, scratch, scratch_bytes, stream);
}

extern "C" int rg_digraph_layer_bwd(int32_t n_src, int32_t n_dst, int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host,
                                    const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel, const int32_t* row_of_dst,
                                    int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld,
                                    const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                                    const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_gate,
                                    float* grad_hidden, float* grad_a_s, void* scratch, size_t scratch_bytes, void* stream) {
  return rgdb::run("rg_digraph_layer_bwd", nullptr, nullptr, n_src, n_dst, n_edges, src_ptr, src_ptr_host, edge_of, dst_of_edge, rel, row_of_dst,
                   n_rela_rows, batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, grad_agg, grad_gate, grad_hidden,
                   grad_a_s, scratch, scratch_bytes, stream);
}

extern "C" int rg_digraph_tlayer_bwd(int32_t n_src, int32_t n_dst, int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host,
                                     const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel, const int32_t* edge_time,
                                     const int32_t* row_of_dst, const int32_t* q_time, int32_t n_rela_rows, int32_t batch, int32_t n_time,
                                     int32_t n_dir, const float* hidden, const float* rela, const float* time_tab, int32_t d, int32_t ld,
                                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                                     const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_gate, float* grad_hidden,
                                     float* grad_a_s_dir, void* scratch, size_t scratch_bytes, void* stream) {
  const rgdb::TimeIn T{edge_time, q_time, time_tab, n_time, n_dir};
  return rgdb::run("rg_digraph_tlayer_bwd", &T, nullptr, n_src, n_dst, n_edges, src_ptr, src_ptr_host, edge_of, dst_of_edge, rel, row_of_dst,
                   n_rela_rows, batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, grad_agg, grad_gate, grad_hidden,
                   grad_a_s_dir, scratch, scratch_bytes, stream);
}
