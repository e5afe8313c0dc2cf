// One message-passing layer over an explicit, destination-segmented edge list (rg_digraph_layer_fwd): the executor behind
// explain.RDigraph.rescore, which re-scores an answer on its r-digraph with some edges masked out.  Every other layer kernel
// enumerates its edges from the graph's CSR and the frontier bitmaps; this one is handed them:
//
//   for every destination o (a CSR row dst_ptr[o] .. dst_ptr[o + 1] of the edge list), b = row_of_dst[o]:
//     for every edge e of the row, in list order, s = src_idx[e], r = rel[e]:
//       alpha_e = sigmoid(w . relu((a_s[s] + a_r[r]) + a_q[b]) + b_alpha)        attn.h attn_acc_fwd / attn_alpha: the forward's float
//       acc    += alpha_e * (hidden[s] + rela[r])
//     agg[o] = acc
//
// Mapping (wave64): a destination is owned by a group of G lanes, G * 4 >= ld floats, so a row is one float4 per lane and a wave
// holds 64 / G destinations.  A round takes G edges of the destination: lane j forms the attention scalar of edge j (and stores it
// to alpha_out), then the group walks the round's edges in order, each lane gathering its float4 of hidden[s] and rela[r], four
// gathers in flight.  All lanes of a wave run the same number of rounds (the longest destination's) with their stores predicated, so
// the lane exchanges never read an inactive lane.
//
// Split rule (the scatter / gather rule for skewed segment lengths): a destination of more than DIGRAPH_CHUNK edges is cut into
// chunks of DIGRAPH_CHUNK edges counted from ITS OWN first edge; every chunk is an item of the same launch that sums into a partial
// row, and a second launch adds the partial rows in chunk order.  A wave per destination alone would run as long as the hub.
// No float atomics; the sums of a destination are formed in list order inside a chunk and in chunk order across chunks, so agg[o]
// has the same bits on every run and does not depend on what else the call carries.
//
// The timed form (rg_digraph_tlayer_fwd, template parameter TIMED; the static instantiation compiles to what it did without it): an
// edge also has a time, a query a time, and the message a third table,
//       n_dir == 3   dt = edge_time[e] - q_time[b], dir = 0 / 1 / 2 for dt < 0 / == 0 / > 0           (rg_tlayer_fwd's rows)
//                    acc += alpha_e * (hidden[3 s + dir] + (rela[dir * n_rela_rows + r] + time_tab[dir * n_time + min(|dt|, n_time - 1)]))
//       n_dir == 1   acc += alpha_e * (hidden[s] + (rela[r] + time_tab[clamp(q_time[b] - edge_time[e], 0, n_time - 1)]))   (rg_xlayer_fwd's)
// alpha_e read from the un-directed s and r as above.  The group then exchanges four values per edge and has twelve gathers in flight.
//
// The gated, replicated form (rg_digraph_layer_fwd_gated, template parameter GATED; static only, and the other instantiations compile
// to what they did without it): the call carries n_rep replicas of the hop, replica k with its own hidden and a_s rows (k * n_src + s)
// and its own outputs (agg rows k * n_dst + o, alpha_out[k * E + e], partial rows k * n_chunks + slot), every index array, rela, a_r,
// a_q and w shared.  An edge has a gate g = fmaf(t[k], gate_hi[e] - gate_lo[e], gate_lo[e]) that multiplies its message:
//       c = g * alpha_e   (rounded once; exactly alpha_e at g == 1)        acc = fmaf(c, hidden[s] + rela[r], acc)
// The gate does not enter alpha_e.  Mapping: an item is a (replica, destination or chunk) pair, item k * n_items + i, so a group works
// exactly as it does in an n_rep = 1 call and a replica's bits do not depend on the others; the group exchanges c where the ungated
// kernel exchanges alpha.  The combine launch has a grid row per replica.
//
// A gate per (replica, edge) (rg_digraph_layer_fwd_gates; learned edge masks): the same instantiation with a replica stride on the
// gate pointers, gate_lo == gate_hi == gate + k * E and t read as 1, so that g = fmaf(1, 0, gate[k * E + e]) is that value and replica
// k has the bits of a one-replica gated call at lo == hi == gate[k].
#include <algorithm>
#include <type_traits>
#include <vector>

#include "attn.h"

namespace rgdg {
namespace {

constexpr int DIGRAPH_CHUNK = RG_DIGRAPH_CHUNK;   // edges per chunk of a cut destination (include/redgnn.h)
constexpr int DG_BLOCK = 256;                     // 4 waves

struct DgArgs {
  int n_dst, n_items;          // items: [0, n_dst) the destinations themselves, then the chunks of the cut ones
  int E, n_src, n_rela_rows, B;
  const int32_t* dst_ptr;
  const int32_t* src_idx;
  const int32_t* rel;
  const int32_t* row_of_dst;
  const int4* chunks;          // [n_items - n_dst] {destination, first edge, end, slot of the partial row}
  const float4* hidden;
  const float4* rela;
  int ld4;
  const float4* a_s;
  const float4* a_r;
  const float4* a_q;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  float4* agg;
  float4* partial;
  float* alpha_out;
};

// what the timed form (rg_digraph_tlayer_fwd) reads on top: kept apart so that the static kernel's arguments stay what they were
struct DgTimedArgs : DgArgs {
  const int32_t* edge_time;    // [E]
  const int32_t* q_time;       // [B]
  const float4* time_tab;      // [n_dir * n_time, ld]
  int n_time, n_dir;           // n_dir 3: interpolation (rows by direction), 1: extrapolation form (one table of lags)
};

// what the gated form (rg_digraph_layer_fwd_gated) reads on top
struct DgGatedArgs : DgArgs {
  int n_rep, n_chunks;         // replicas; chunks of ONE replica (replica k's partial rows start at k * n_chunks)
  const float* t;              // [n_rep], or nullptr: 1 (the per-replica form)
  const float* gate_lo;        // [E] or nullptr: 0
  const float* gate_hi;        // [E] or nullptr: 1
  int gate_rep;                // replica k's gates start k * gate_rep floats further on (n_rep * E fits int32): 0, the shared pair, or
                               // E with gate_lo == gate_hi (rg_digraph_layer_fwd_gates)
};

template <bool TIMED, bool GATED>
using DgArgsOf = std::conditional_t<GATED, DgGatedArgs, std::conditional_t<TIMED, DgTimedArgs, DgArgs>>;

__device__ __forceinline__ int clampi(int x, int hi) { return min(max(x, 0), hi); }

template <int G, int AP4, bool TIMED, bool GATED>
__global__ __launch_bounds__(DG_BLOCK) void digraph_fwd_kernel(DgArgsOf<TIMED, GATED> A) {
  static_assert(!(TIMED && GATED), "the gated form is static");
  constexpr int PER_WAVE = 64 / G;
  const int lane = threadIdx.x & 63;
  const int lane_g = lane & (G - 1), gbase = lane & ~(G - 1);
  const int wave = blockIdx.x * (DG_BLOCK / 64) + (threadIdx.x >> 6);
  int item = wave * PER_WAVE + lane / G;
  int rep = 0;                                           // GATED: the item's replica, and the item inside it
  if constexpr (GATED) {
    rep = item / A.n_items;
    item -= rep * A.n_items;
    if (rep >= A.n_rep) { rep = 0; item = A.n_items; }   // past the last replica: no work
  }
  const bool row_lane = lane_g < A.ld4;
  const int lane_c = row_lane ? lane_g : A.ld4 - 1;      // loads never branch: idle lanes re-read the last float4

  // the item's destination, edge range and output row; an item without work keeps beg == end and stores nothing
  int o = 0, beg = 0, end = 0;
  float4* out = nullptr;
  if (item < A.n_dst) {
    o = item;
    const int lo = clampi(A.dst_ptr[o], A.E), hi = clampi(A.dst_ptr[o + 1], A.E);
    if (hi - lo <= DIGRAPH_CHUNK) {                      // (a cut destination is written by the combine pass)
      beg = lo; end = max(hi, lo);
      out = A.agg + (int64_t)o * A.ld4;
      if constexpr (GATED) out += (int64_t)rep * A.n_dst * A.ld4;
    }
  } else if (item < A.n_items) {
    const int4 c = A.chunks[item - A.n_dst];
    o = clampi(c.x, A.n_dst - 1);
    beg = clampi(c.y, A.E); end = min(max(clampi(c.z, A.E), beg), beg + DIGRAPH_CHUNK);
    out = A.partial + (int64_t)c.w * A.ld4;
    if constexpr (GATED) out += (int64_t)rep * A.n_chunks * A.ld4;
  }
  const int b = clampi(A.row_of_dst[o], A.B - 1);
  const float b_alpha = A.b_alpha[0];
  const float4* aq_p = A.a_q + (int64_t)b * AP4;
  int qt = 0;
  if constexpr (TIMED) qt = A.q_time[b];
  // GATED: the replica's rows of hidden and a_s, its alpha_out and its t
  const float4* hidden_p = A.hidden;
  const float4* as_tab = A.a_s;
  float* alpha_out = A.alpha_out;
  float t_rep = 1.f;
  if constexpr (GATED) {
    hidden_p += (int64_t)rep * A.n_src * A.ld4;
    as_tab += (int64_t)rep * A.n_src * AP4;
    if (alpha_out) alpha_out += (int64_t)rep * A.E;
    if (A.t) t_rep = A.t[rep];
  }
  int gate_at = 0;                                       // GATED: where the replica's gates start (n_rep * E fits int32)
  if constexpr (GATED) gate_at = rep * A.gate_rep;

  float4 acc = rg::f4zero();
  for (int c0 = beg; __any(c0 < end); c0 += G) {
    // ---- one edge per lane: indices and the attention scalar --------------------------------------------------
    const int c = c0 + lane_g;
    const bool valid = c < end;
    int s = 0, r = 0, trow = 0;
    float alpha = 0.f;
    if (valid) {
      s = clampi(A.src_idx[c], A.n_src - 1);
      r = clampi(A.rel[c], A.n_rela_rows - 1);
      float z = b_alpha;
#pragma clang loop unroll_count(AP4 >= 8 ? 2 : AP4)
      for (int k = 0; k < AP4; ++k)
        rg::attn_acc_fwd(z, rg::attn_w4(A.w_alpha, A.attn_dim, k), as_tab[(int64_t)s * AP4 + k], A.a_r[(int64_t)r * AP4 + k], aq_p[k]);
      alpha = rg::attn_alpha(z);
      if (alpha_out) alpha_out[c] = alpha;
      if constexpr (GATED) {                             // from here on alpha is the message's coefficient c = g * alpha_e
        const float lo = A.gate_lo ? A.gate_lo[gate_at + c] : 0.f, hi = A.gate_hi ? A.gate_hi[gate_at + c] : 1.f;
        alpha = fmaf(t_rep, hi - lo, lo) * alpha;
      }
      if constexpr (TIMED) {
        // the rows of the message, as layer_fwd_kernel.h forms them (the attention above read the un-directed s and r); 64-bit
        // differences, so that no pair of times overflows, and the time row clamped into its table
        const int64_t et = A.edge_time[c];
        if (A.n_dir == 3) {
          const int64_t dt = et - qt;
          const int dir = dt > 0 ? 2 : (dt == 0 ? 1 : 0);
          s = s * 3 + dir;
          r = dir * A.n_rela_rows + r;
          trow = dir * A.n_time + (int)min(dt < 0 ? -dt : dt, (int64_t)(A.n_time - 1));
        } else {
          trow = (int)min(max((int64_t)qt - et, (int64_t)0), (int64_t)(A.n_time - 1));
        }
      }
    }
    const int cnt = min(max(end - c0, 0), G);
    // ---- the round's edges in order, every lane its float4 of the row; four edges' gathers in flight -----------
    for (int j = 0; __any(j < cnt); j += 4) {
      int su[4], ru[4], tu[4];
      float al[4];
      float4 hv[4], rv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {      // (slots past cnt hold s = r = 0: row 0 is read and not used)
        const int from = gbase + ((j + u) & (G - 1));
        su[u] = __shfl(s, from, 64);
        ru[u] = __shfl(r, from, 64);
        al[u] = __shfl(alpha, from, 64);
        if constexpr (TIMED) tu[u] = __shfl(trow, from, 64);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) hv[u] = hidden_p[(int64_t)su[u] * A.ld4 + lane_c];
#pragma unroll
      for (int u = 0; u < 4; ++u) rv[u] = A.rela[(int64_t)ru[u] * A.ld4 + lane_c];
      if constexpr (TIMED) {             // rela[rrow] + time_tab[trow] first, then hidden: layer_fwd_kernel.h's association
        float4 tv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tv[u] = A.time_tab[(int64_t)tu[u] * A.ld4 + lane_c];
#pragma unroll
        for (int u = 0; u < 4; ++u) { rv[u].x += tv[u].x; rv[u].y += tv[u].y; rv[u].z += tv[u].z; rv[u].w += tv[u].w; }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (j + u < cnt) {
          acc.x = fmaf(al[u], hv[u].x + rv[u].x, acc.x);
          acc.y = fmaf(al[u], hv[u].y + rv[u].y, acc.y);
          acc.z = fmaf(al[u], hv[u].z + rv[u].z, acc.z);
          acc.w = fmaf(al[u], hv[u].w + rv[u].w, acc.w);
        }
      }
    }
  }
  if (out && row_lane) out[lane_g] = acc;
}

// agg[o] of the cut destinations: their chunks' partial rows added in chunk order, the first one initialising the sum
// (gated form: grid row k is replica k, its partial rows and its agg rows partial_rep / agg_rep float4 further on)
__global__ void digraph_combine_kernel(const int4* __restrict__ hubs, int n_hubs, const float4* __restrict__ partial,
                                       float4* __restrict__ agg, int ld4, int64_t partial_rep, int64_t agg_rep) {
  partial += blockIdx.y * partial_rep;
  agg += blockIdx.y * agg_rep;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t h = tid / ld4;
  const int c = (int)(tid - h * ld4);
  if (h >= n_hubs) return;
  const int4 hub = hubs[h];                              // {destination, first slot, chunks, -}
  const float4* p = partial + (int64_t)hub.y * ld4 + c;
  float4 acc = p[0];
  for (int k = 1; k < hub.z; ++k) {
    const float4 v = p[(int64_t)k * ld4];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  agg[(int64_t)hub.x * ld4 + c] = acc;
}

// the cut destinations of a CSR on the host: how many, and how many chunks they make
void count_cuts(const int32_t* ptr, int32_t n_dst, int64_t* n_hubs, int64_t* n_chunks) {
  *n_hubs = *n_chunks = 0;
  for (int32_t o = 0; o < n_dst; ++o) {
    const int64_t len = (int64_t)ptr[o + 1] - ptr[o];
    if (len > DIGRAPH_CHUNK) { ++*n_hubs; *n_chunks += rg::ceil_div(len, DIGRAPH_CHUNK); }
  }
}

size_t list_bytes(int64_t n_hubs, int64_t n_chunks) { return rg::align_up((size_t)(n_hubs + n_chunks) * sizeof(int4), 256); }

template <int G, int AP4, bool TIMED, bool GATED = false>
int launch(const DgArgsOf<TIMED, GATED>& A, hipStream_t s) {
  int64_t items = A.n_items;
  if constexpr (GATED) items *= A.n_rep;
  const int64_t waves = rg::ceil_div(items, 64 / G);
  hipLaunchKernelGGL((digraph_fwd_kernel<G, AP4, TIMED, GATED>), dim3((unsigned)rg::ceil_div(waves, DG_BLOCK / 64)), dim3(DG_BLOCK), 0, s, A);
  RG_LAUNCH_CHECK();
  return 0;
}

// the time arguments of rg_digraph_tlayer_fwd; nullptr: the static entry point
struct TimeIn {
  const int32_t* edge_time;
  const int32_t* q_time;
  const float* time_tab;
  int32_t n_time, n_dir;
};

// the gate arguments of rg_digraph_layer_fwd_gated / _gates; nullptr: the ungated entry points.  per_rep (rg_digraph_layer_fwd_gates):
// gate_lo == gate_hi is the [n_rep, E] array and t is not read, so that the kernel's fmaf(1, 0, lo) is the array's value
struct GateIn {
  int32_t n_rep;
  const float* t;
  const float* gate_lo;
  const float* gate_hi;
  bool per_rep;
};

size_t scratch_need(int64_t n_hubs, int64_t n_chunks, int32_t ld, int64_t n_rep) {
  return n_hubs ? list_bytes(n_hubs, n_chunks) + rg::align_up((size_t)(n_rep * n_chunks) * ld * sizeof(float), 256) : 0;
}

// every entry point: every check, then the chunk list, the layer launch and the combine launch
int run(const char* who, const TimeIn* T, const GateIn* Q, int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr, const int32_t* dst_ptr_host,
        const int32_t* src_idx, const int32_t* rel, const int32_t* row_of_dst, int32_t n_src, int32_t n_rela_rows, int32_t batch,
        const float* hidden, const float* rela, int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q, int32_t ap,
        const float* w_alpha, const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out, void* scratch,
        size_t scratch_bytes, void* stream) {
  RG_CHECK(n_dst >= 0 && n_edges >= 0 && n_edges < ((int64_t)1 << 31), "%s: n_dst=%d n_edges=%lld (need 0 <= n_dst, 0 <= n_edges < 2^31)",
           who, n_dst, (long long)n_edges);
  RG_CHECK(n_src >= 0 && n_rela_rows >= 0 && batch >= 0, "%s: n_src=%d n_rela_rows=%d batch=%d (negative size)", who, n_src, n_rela_rows,
           batch);
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
  if (n_dst == 0) {
    RG_CHECK(n_edges == 0, "%s: %lld edges without a destination", who, (long long)n_edges);
    return 0;
  }
  RG_CHECK(dst_ptr_host, "%s: NULL argument (dst_ptr_host)", who);
  RG_CHECK(dst_ptr_host[0] == 0, "%s: dst_ptr starts at %d, not 0", who, dst_ptr_host[0]);
  for (int32_t o = 0; o < n_dst; ++o)
    RG_CHECK(dst_ptr_host[o + 1] >= dst_ptr_host[o], "%s: dst_ptr decreases at destination %d", who, o);
  RG_CHECK(dst_ptr_host[n_dst] == n_edges, "%s: dst_ptr ends at %d, not at the number of edges %lld", who, dst_ptr_host[n_dst],
           (long long)n_edges);
  if (n_edges == 0) return 0;                            // nothing to sum and nothing launched: the caller owns agg_out
  RG_CHECK(dst_ptr && src_idx && rel && row_of_dst && hidden && rela && a_s && a_r && a_q && w_alpha && b_alpha && agg_out,
           "%s: NULL argument", who);
  RG_CHECK(!T || (T->edge_time && T->q_time && T->time_tab), "%s: NULL argument (edge_time, q_time or time_tab)", who);
  RG_CHECK(n_src > 0 && n_rela_rows > 0 && batch > 0, "%s: edges but n_src=%d n_rela_rows=%d batch=%d", who, n_src, n_rela_rows, batch);
  RG_CHECK((((uintptr_t)hidden | (uintptr_t)rela | (uintptr_t)a_s | (uintptr_t)a_r | (uintptr_t)a_q | (uintptr_t)agg_out |
             (uintptr_t)scratch | (uintptr_t)(T ? T->time_tab : nullptr)) & 15) == 0, "%s: float buffers must be 16-B aligned", who);
  int64_t n_hubs, n_chunks;
  count_cuts(dst_ptr_host, n_dst, &n_hubs, &n_chunks);
  RG_CHECK(n_rep * ((int64_t)n_dst + n_chunks) < ((int64_t)1 << 31) - 64, "%s: %lld items overflow int32", who,
           (long long)(n_rep * (n_dst + n_chunks)));
  const size_t need = scratch_need(n_hubs, n_chunks, ld, n_rep);
  RG_CHECK(need == 0 || (scratch && scratch_bytes >= need), "%s: scratch %zu B < required %zu B", who, scratch ? scratch_bytes : (size_t)0,
           need);

  DgTimedArgs A;
  A.n_dst = n_dst; A.n_items = (int)(n_dst + n_chunks); A.E = (int)n_edges; A.n_src = n_src; A.n_rela_rows = n_rela_rows; A.B = batch;
  A.dst_ptr = dst_ptr; A.src_idx = src_idx; A.rel = rel; A.row_of_dst = row_of_dst;
  A.hidden = (const float4*)hidden; A.rela = (const float4*)rela; A.ld4 = ld / 4;
  A.a_s = (const float4*)a_s; A.a_r = (const float4*)a_r; A.a_q = (const float4*)a_q;
  A.w_alpha = w_alpha; A.b_alpha = b_alpha; A.attn_dim = attn_dim;
  A.agg = (float4*)agg_out; A.alpha_out = alpha_out;
  A.edge_time = T ? T->edge_time : nullptr; A.q_time = T ? T->q_time : nullptr; A.time_tab = T ? (const float4*)T->time_tab : nullptr;
  A.n_time = T ? T->n_time : 0; A.n_dir = T ? T->n_dir : 0;
  int4* hubs_dev = (int4*)scratch;
  A.chunks = hubs_dev + n_hubs;
  A.partial = n_hubs ? (float4*)((char*)scratch + list_bytes(n_hubs, n_chunks)) : nullptr;
  // every argument error is out before anything is enqueued: the width dispatch is probed first
  if (rg::with_ap4(ap / 4, who, [](auto) { return 0; })) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (n_hubs) {
    std::vector<int4> list((size_t)(n_hubs + n_chunks));
    int64_t h = 0, slot = 0;
    for (int32_t o = 0; o < n_dst; ++o) {
      const int32_t lo = dst_ptr_host[o], hi = dst_ptr_host[o + 1];
      if (hi - lo <= DIGRAPH_CHUNK) continue;
      const int n_c = (int)rg::ceil_div(hi - lo, DIGRAPH_CHUNK);
      list[h++] = make_int4(o, (int)slot, n_c, 0);
      for (int k = 0; k < n_c; ++k, ++slot)
        list[n_hubs + slot] = make_int4(o, lo + k * DIGRAPH_CHUNK, std::min(hi, lo + (k + 1) * DIGRAPH_CHUNK), (int)slot);
    }
    // (a copy from pageable memory: the runtime is done with the vector when the call returns)
    RG_HIP(hipMemcpyAsync(hubs_dev, list.data(), list.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  }
  const int rc = rg::with_g(A.ld4, [&](auto g) {
    return rg::with_ap4(ap / 4, who, [&](auto a4) {
      if (T) return launch<decltype(g)::value, decltype(a4)::value, true>(A, s);
      if (Q) {
        DgGatedArgs GA;
        static_cast<DgArgs&>(GA) = A;
        GA.n_rep = (int)n_rep; GA.n_chunks = (int)n_chunks; GA.t = Q->t; GA.gate_lo = Q->gate_lo; GA.gate_hi = Q->gate_hi;
        GA.gate_rep = Q->per_rep ? (int)n_edges : 0;
        return launch<decltype(g)::value, decltype(a4)::value, false, true>(GA, s);
      }
      return launch<decltype(g)::value, decltype(a4)::value, false>(A, s);
    });
  });
  if (rc) return rc;
  if (n_hubs) {
    const int64_t threads = n_hubs * A.ld4;
    hipLaunchKernelGGL(digraph_combine_kernel, dim3((unsigned)rg::ceil_div(threads, 256), (unsigned)n_rep), dim3(256), 0, s, hubs_dev,
                       (int)n_hubs, (const float4*)A.partial, A.agg, A.ld4, n_chunks * A.ld4, (int64_t)n_dst * A.ld4);
    RG_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace
}  // namespace rgdg

extern "C" size_t rg_digraph_layer_fwd_scratch_bytes(const int32_t* dst_ptr_host, int32_t n_dst, int32_t ld) {
  if (!dst_ptr_host || n_dst <= 0 || ld <= 0) return 0;
  for (int32_t o = 0; o < n_dst; ++o)
    if (dst_ptr_host[o + 1] < dst_ptr_host[o]) return 0;
  int64_t n_hubs, n_chunks;
  rgdg::count_cuts(dst_ptr_host, n_dst, &n_hubs, &n_chunks);
  if (n_hubs == 0) return 0;
  return rgdg::scratch_need(n_hubs, n_chunks, ld, 1);
}

extern "C" size_t rg_digraph_layer_fwd_gated_scratch_bytes(const int32_t* dst_ptr_host, int32_t n_dst, int32_t ld, int32_t n_rep) {
  if (!dst_ptr_host || n_dst <= 0 || ld <= 0 || n_rep < 1) return 0;
  for (int32_t o = 0; o < n_dst; ++o)
    if (dst_ptr_host[o + 1] < dst_ptr_host[o]) return 0;
  int64_t n_hubs, n_chunks;
  rgdg::count_cuts(dst_ptr_host, n_dst, &n_hubs, &n_chunks);
  return rgdg::scratch_need(n_hubs, n_chunks, ld, n_rep);
}

extern "C" int rg_digraph_layer_fwd_gated(int32_t n_rep, const float* t, const float* gate_lo, const float* gate_hi, int32_t n_dst,
                                          int64_t n_edges, const int32_t* dst_ptr, const int32_t* dst_ptr_host, const int32_t* src_idx,
                                          const int32_t* rel, const int32_t* row_of_dst, int32_t n_src, int32_t n_rela_rows, int32_t batch,
                                          const float* hidden, const float* rela, int32_t d, int32_t ld, const float* a_s, const float* a_r,
                                          const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                                          float* agg_out, float* alpha_out, void* scratch, size_t scratch_bytes, void* stream) {
  const rgdg::GateIn Q{n_rep, t, gate_lo, gate_hi, false};
  return rgdg::run("rg_digraph_layer_fwd_gated", nullptr, &Q, n_dst, n_edges, dst_ptr, dst_ptr_host, src_idx, rel, row_of_dst, n_src,
                   n_rela_rows, batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, agg_out, alpha_out, scratch,
                   scratch_bytes, stream);
}

extern "C" int rg_digraph_layer_fwd_gates(int32_t n_rep, const float* gate, int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr,
                                          const int32_t* dst_ptr_host, const int32_t* src_idx, const int32_t* rel, const int32_t* row_of_dst,
                                          int32_t n_src, int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela,
                                          int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                                          const float* w_alpha, const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out,
                                          void* scratch, size_t scratch_bytes, void* stream) {
  const rgdg::GateIn Q{n_rep, nullptr, gate, gate, true};
  return rgdg::run("rg_digraph_layer_fwd_gates", nullptr, &Q, n_dst, n_edges, dst_ptr, dst_ptr_host, src_idx, rel, row_of_dst, n_src,
                   n_rela_rows, batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, agg_out, alpha_out, scratch,
                   scratch_bytes, stream);
}

extern "C" int rg_digraph_layer_fwd(int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr, const int32_t* dst_ptr_host,
                                    const int32_t* src_idx, const int32_t* rel, const int32_t* row_of_dst, int32_t n_src,
                                    int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld,
                                    const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                                    const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out, void* scratch,
                                    size_t scratch_bytes, void* stream) {
  return rgdg::run("rg_digraph_layer_fwd", nullptr, nullptr, n_dst, n_edges, dst_ptr, dst_ptr_host, src_idx, rel, row_of_dst, n_src, n_rela_rows,
                   batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, agg_out, alpha_out, scratch, scratch_bytes,
                   stream);
}

extern "C" int rg_digraph_tlayer_fwd(int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr, const int32_t* dst_ptr_host,
                                     const int32_t* src_idx, const int32_t* rel, const int32_t* edge_time, const int32_t* row_of_dst,
                                     const int32_t* q_time, int32_t n_src, int32_t n_rela_rows, int32_t batch, int32_t n_time,
                                     int32_t n_dir, const float* hidden, const float* rela, const float* time_tab, int32_t d, int32_t ld,
                                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                                     const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out, void* scratch,
                                     size_t scratch_bytes, void* stream) {
  const rgdg::TimeIn T{edge_time, q_time, time_tab, n_time, n_dir};
  return rgdg::run("rg_digraph_tlayer_fwd", &T, nullptr, n_dst, n_edges, dst_ptr, dst_ptr_host, src_idx, rel, row_of_dst, n_src, n_rela_rows,
                   batch, hidden, rela, d, ld, a_s, a_r, a_q, ap, w_alpha, b_alpha, attn_dim, agg_out, alpha_out, scratch, scratch_bytes,
                   stream);
}
