// Fused relational message passing, forward, for hop 0 of a query batch (walk code 8 of rg_layer_fwd).
//
// At level 1 every query b has ONE source, its subject s_b (node id b of level 0), so the hop's edges are exactly the out-edges of s_b.
// The general walks find them from the destination side: they sweep (query group x pack) items of the CSR-by-tail that mostly hold
// nothing, cut hub destinations into partial rows and add those in a second launch.  Here the edges are read where they are:
//
//   for every query b:   s = sub[b];  the list out_bt[out_ptr[s] .. out_ptr[s+1]) is ordered by (tail, CSR-by-tail position)
//     for every run of equal tail t in it:                      (a run = all edges s -> t, in the order the CSR-by-tail lists them)
//       alpha_e = sigmoid(w . relu(a_s[b] + a_r[r] + a_q[b]) + b_alpha)          (rg::attn_acc_fwd / rg::attn_alpha: the walks' alpha)
//       acc    += alpha_e * (hidden[b] + rela[r])                                in list order
//       agg[rank of (b, t) in level 1] = acc
//
// The sum of a destination is formed in one place, hubs included: no partial rows, no `written` flags, no combine_kernel, no atomics.
// It is bit for bit the sum of the other walks.  Those add a destination's edges in CSR-by-tail order - which is the run's order - and
// a destination of in-degree > RG_VROW_MAX in 128-entry segments: one fma chain from zero per segment, the segments' rows then added in
// segment order (combine_kernel; an empty segment adds +0).  A run that spans segments of its destination (several edges s -> t whose
// CSR positions lie in different segments) is therefore summed here segment by segment as well: out_bt_pos gives the position.
//
// Mapping: a group of G lanes (G * 4 >= ld floats, one float4 of the row per lane) takes a chunk of SRC1_CHUNK list entries; a chunk
// owns the runs that START inside it (it skips the tail of a run begun before it and finishes its own last run past its end), so a
// run is never cut and a hub subject of out-degree 17k is 500 independent chunks.  Per G entries: one entry per lane (list entry, rank
// of its tail in the level-1 bitmap, segment, alpha), staged in an LDS strip; then the group walks the strip in order, four relation
// rows in flight.  grid = (B, Y): the groups of the Y workgroups of a query stride over its chunks; workgroups beyond a query's list
// leave at once.
#include "attn.h"
#include "layer_fwd_src1.h"

namespace rgsrc1 {
namespace {

constexpr int SRC1_BLOCK = 256;
constexpr int SRC1_CHUNK = 32;
constexpr int SRC1_MAX_Y = 8;

template <int G, int AP4, bool PACKED>
__global__ __launch_bounds__(SRC1_BLOCK) void layer_fwd_src1_kernel(Src1Args A) {
  __shared__ float4 stage[SRC1_BLOCK];                   // per group a strip of G tuples {rank of the tail, rel, alpha, segment}
  constexpr int NG = SRC1_BLOCK / G;
  const int b = blockIdx.x;
  const int s = A.sub[b];
  if (s < 0) return;
  const int beg = A.out_ptr[s], end = A.out_ptr[s + 1];
  const int n_chunks = (end - beg + SRC1_CHUNK - 1) / SRC1_CHUNK;
  if ((int)blockIdx.y * NG >= n_chunks) return;

  const int lane = threadIdx.x & 63;
  const int lane_g = lane & (G - 1), grp = threadIdx.x / G;
  float4* my_stage = stage + grp * G;
  const bool row_lane = lane_g < A.ld4;
  const int lane_c = row_lane ? lane_g : A.ld4 - 1;      // loads never branch: idle lanes re-read the last float4
  const float4 hv = A.hidden[(int64_t)b * A.ld4 + lane_c];
  const float b_alpha = A.b_alpha[0];
  const int2* bm_row = A.bm_new + (int64_t)b * A.W;
  const float4* as_p = A.a_s + (int64_t)b * AP4;
  const float4* aq_p = A.a_q + (int64_t)b * AP4;

  auto tail_of = [&](int i) -> int {
    if constexpr (PACKED) return (int)(A.list_pk[i] & 0xFFFFF);
    else return A.list_rt[i].y;
  };

  for (int c = (int)blockIdx.y * NG + grp; c < n_chunks; c += (int)gridDim.y * NG) {
    const int lo = beg + c * SRC1_CHUNK, hi = min(lo + SRC1_CHUNK, end);
    // the run the previous chunk finishes: skipped here (by the rank of its tail; -1 = none)
    int skip_o = -1;
    if (c > 0) {
      const int tp = tail_of(lo - 1);
      const int2 wp = bm_row[tp >> 5];
      if (rg::bm_has(wp, tp)) skip_o = rg::bm_rank(wp, tp);
    }
    int cur_o = -2, cur_seg = 0;
    bool started = false, done = false;
    float4 acc = rg::f4zero(), total = rg::f4zero();
    auto close_segment = [&]() {
      if (!started) { total = acc; started = true; }
      else { total.x += acc.x; total.y += acc.y; total.z += acc.z; total.w += acc.w; }
    };
    auto close_row = [&]() {
      if (cur_o < 0) return;
      close_segment();
      if (row_lane) A.agg[(int64_t)cur_o * A.ld4 + lane_g] = total;
    };

    for (int i0 = lo; i0 < end && !done; i0 += G) {
      // ---- phase 1: one list entry per lane ---------------------------------------------------------------------------------
      const int i = i0 + lane_g;
      int o = -1, r = 0, seg = 0;
      float alpha = 0.f;
      if (i < end) {
        int t;
        if constexpr (PACKED) { const uint32_t pk = A.list_pk[i]; t = pk & 0xFFFFF; r = pk >> 20; }
        else { const int2 rt = A.list_rt[i]; r = rt.x; t = rt.y; }
        const int pos = A.list_pos[i];
        const int2 wp = bm_row[t >> 5];
        const int ip0 = A.in_ptr[t], ip1 = A.in_ptr[t + 1];
        if (rg::bm_has(wp, t)) {
          o = rg::bm_rank(wp, t);
          seg = ip1 - ip0 > RG_VROW_MAX ? (pos - ip0) / RG_VROW_MAX : 0;
          float z = b_alpha;
#pragma clang loop unroll_count(AP4 >= 8 ? 2 : AP4)
          for (int k = 0; k < AP4; ++k) {
            const float4 as = as_p[k];
            const float4 ar = A.a_r[(int64_t)r * AP4 + k];
            const float4 w = rg::attn_w4(A.w_alpha, A.attn_dim, k);
            const float4 q = aq_p[k];
            rg::attn_acc_fwd(z, w, as, ar, q);
          }
          alpha = rg::attn_alpha(z);
        }
      }
      rg::strip_fence<false>();
      my_stage[lane_g] = make_float4(__int_as_float(o), __int_as_float(r), alpha, __int_as_float(seg));
      rg::strip_fence<false>();

      // ---- phase 2: the group walks the strip in list order, four relation rows in flight ---------------------------------------
      const int n = min(G, end - i0);
      for (int k0 = 0; k0 < n && !done; k0 += 4) {
        float4 tp[4], rv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) tp[u] = my_stage[min(k0 + u, G - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) rv[u] = A.rela[(int64_t)__float_as_int(tp[u].y) * A.ld4 + lane_c];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          if (k0 + u >= n || done) continue;
          const int ou = __float_as_int(tp[u].x), su = __float_as_int(tp[u].w);
          if (i0 + k0 + u >= hi && ou != cur_o) { done = true; continue; }     // past the chunk and its last run is over
          if (ou < 0) continue;
          if (skip_o >= 0) {
            if (ou == skip_o) continue;
            skip_o = -1;
          }
          if (ou != cur_o) {
            close_row();
            cur_o = ou; cur_seg = su; started = false; acc = rg::f4zero();
          } else if (su != cur_seg) {
            close_segment();
            cur_seg = su; acc = rg::f4zero();
          }
          const float al = tp[u].z;
          acc.x = fmaf(al, hv.x + rv[u].x, acc.x);
          acc.y = fmaf(al, hv.y + rv[u].y, acc.y);
          acc.z = fmaf(al, hv.z + rv[u].z, acc.z);
          acc.w = fmaf(al, hv.w + rv[u].w, acc.w);
        }
      }
    }
    close_row();
  }
}

template <int G, int AP4>
int launch2(const Src1Args& A, int max_out_deg, hipStream_t s) {
  constexpr int NG = SRC1_BLOCK / G;
  const int y = (int)std::min<int64_t>(std::max<int64_t>(rg::ceil_div(rg::ceil_div(max_out_deg, SRC1_CHUNK), NG), 1), SRC1_MAX_Y);
  if (A.list_pk) hipLaunchKernelGGL((layer_fwd_src1_kernel<G, AP4, true>), dim3(A.B, y), dim3(SRC1_BLOCK), 0, s, A);
  else hipLaunchKernelGGL((layer_fwd_src1_kernel<G, AP4, false>), dim3(A.B, y), dim3(SRC1_BLOCK), 0, s, A);
  RG_LAUNCH_CHECK();
  return 0;
}

}  // namespace

int launch(const Src1Args& A, int ld4, int ap4, int max_out_deg, hipStream_t s) {
  return rg::with_g(ld4, [&](auto g) {
    return rg::with_ap4(ap4, "rg_layer_fwd", [&](auto ap) { return launch2<decltype(g)::value, decltype(ap)::value>(A, max_out_deg, s); });
  });
}

}  // namespace rgsrc1
