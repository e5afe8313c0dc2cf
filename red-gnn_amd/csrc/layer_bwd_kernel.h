// Fused relational message passing, backward: the adjoint of layer_fwd_kernel.h for the static layer (layer_bwd.hip) and the
// temporal interpolation and extrapolation layers (tlayer_bwd.hip).
// Replaces what autograd replays for Static/transductive/models.py:29-39 (index / add / Linear x3 / sigmoid / mul / scatter) and
// Temporal/interpolation/model_cuda.py:149-160,192 on E-row temporaries.  Source-pull formulation: every node (b,h) of the
// previous frontier walks its KG out-edges (CSR by head, cut into length-sorted virtual rows exactly as the forward's CSR by
// tail); every out-edge of a visited node is an edge of the hop, its destination id is the popcount rank of (b,t) in the new
// frontier.
//
//   per edge e=(s,r,o):   z = relu(a_s[s] + a_r[r] + a_q[b]);  alpha = sigma(w.z + b_alpha)
//     STATIC    m = H[s] + Rel[r]
//     TEMPORAL  m = hidden_dir[3 s + dir] + rela_dir[dir * n_rela_rows + r] + time_dir[dir * n_time + |dt|],  dt = time(e) - q_time[b]
//     WINDOWED  the extrapolation layer (Temporal/extrapolation/model_cuda_new_embedding.py:186-239): an edge's time field is its
//               data row, valid for query b inside the row window [win_lo[b], win_hi[b]) only (self-loops, row >= n_data, always);
//               one direction (every edge lies in the past), m = hidden_p[s] + rela_p[r] + time_p[trow],
//               trow = clamp(q_time[b] - row_time[row], 0, n_time - 1)  (self-loops: q_time[b] - loop_time[b])
//     g_alpha = <G[o], m>                    g_p  = g_alpha * alpha (1 - alpha)     g_z = g_p * w * 1[z>0]
//     dH[s]   += alpha G[o]   (registers, one store per source row / segment: deterministic; TEMPORAL: one accumulator per direction)
//     dA_s[s] += g_z          (registers -> one store per source / segment)
//     dA_r[r] += g_z          (LDS)            dw += g_p relu(z), db += g_p (STATIC)   (registers -> block reduce)
//   dA_q[b] = sum of dA_s over the nodes of query b is left to the caller (a segment sum).
// The relation (and time) table gradients are the key-major pass of key_bwd_kernel.h; the attention scalar and the bitmap lookup
// are attn.h's; the projections a_s = H Ws^T etc. and the direction linears are differentiated by the caller (dense GEMMs).
// Work distribution: walk.h (in-order per-XCD queues; grad_agg rows of the query being processed stay in L2).
#pragma once
#include "walk.h"

namespace rgbwd {
namespace {   // internal linkage: the header is instantiated by layer_bwd.hip and tlayer_bwd.hip

enum Layer { STATIC, TEMPORAL, WINDOWED };

// direction rows per source node
constexpr int dir_rows(Layer L) { return L == TEMPORAL ? 3 : 1; }

struct BwdArgs {
  rg::WalkArgs walk;   // items tested against the OLD frontier (sources); vrows = CSR-by-head segments
  const int2* out_rt;
  const uint32_t* out_pk = nullptr;   // STATIC: packed (rel << 20 | tail) entries, if the graph has them
  const int2* bm_new;
  int W;
  const float4* hidden;     // [dir_rows * N_old][ld4]  (row dir_rows * s + dir)
  const float4* rela;       // STATIC: [n_rela_rows][ld4];  TEMPORAL: [3 * n_rela_rows][ld4];  WINDOWED: [n_rela_rows][ld4]
  int ld4;
  const float4* a_s;
  const float4* a_r;
  const float4* a_q;
  const float* w_alpha;
  const float* b_alpha;
  int attn_dim;
  int n_rela_rows;
  const float4* grad_agg;
  float4* g_hidden;         // [N_old][dir_rows * ld4]
  float4* g_hidden_part;    // [B * n_slots][dir_rows * ld4]
  float4* g_as;
  float4* g_as_part;        // [B * n_slots][AP4]
  float* g_ar;              // [n_rela_rows][ap]
  float* g_w;
  float* g_b = nullptr;     // STATIC
  int kpg = 1;              // STATIC: walk.h items per lane group of the dense walk (8 on short-row graphs)
  // TEMPORAL, WINDOWED
  const int32_t* out_time = nullptr;   // time id (WINDOWED: data row) of every CSR-by-head entry
  const int32_t* q_time = nullptr;
  const float4* time_tab = nullptr;    // TEMPORAL: [3 * n_time][ld4];  WINDOWED: [n_time][ld4]
  int n_time = 0;
  // WINDOWED
  const int32_t* win_lo = nullptr;
  const int32_t* win_hi = nullptr;
  const int32_t* row_time = nullptr;
  const int32_t* loop_time = nullptr;
  int n_data = 0;
};

constexpr int BWD_BLOCK = 512;

// RELA_LDS (STATIC): the rela rows sit in LDS; the temporal tables have 3x the rows and are read from L2.
// KPG: items per lane group and block step of the dense walk (walk.h): 8 on graphs of short rows, as in the forward.
// (AP4 >= 4, attn_dim > 12: 4 x AP4 float4 of per-edge attention state; 256 VGPRs instead of spilling at 128)
template <int G, int AP4, bool PACKED, bool DENSE, bool RELA_LDS, int KPG, Layer L>
__global__ __launch_bounds__(BWD_BLOCK, AP4 >= 4 ? 2 : 4) void layer_bwd_kernel(BwdArgs A) {
  extern __shared__ float4 lds[];
  constexpr int BLOCK = BWD_BLOCK;
  constexpr int ND = dir_rows(L);
  // phase 2: edges per group step; a temporal edge gathers three rows (grad_agg, rela_dir, time_dir)
  constexpr int U = L == STATIC ? 4 : 2;
  const int nr = A.n_rela_rows;
  float4* stage = lds;                      // [BLOCK] {o -> g_alpha, rela row, alpha, time row * 4 + dir}
  float4* ar_l = stage + BLOCK;             // [nr][AP4]
  float4* w_l = ar_l + nr * AP4;            // [AP4]
  float4* gar_l = w_l + AP4;                // [nr][AP4]   grad a_r
  float4* red_l = gar_l + nr * AP4;         // [(BLOCK/64)][AP4 + 1] block reduction of dw, db
  float4* rela_l = red_l + (BLOCK / 64) * (AP4 + 1);                        // [nr][G]  (RELA_LDS)
  int4* recs = reinterpret_cast<int4*>(rela_l + (RELA_LDS ? nr * G : 0));   // [BLOCK] (SPARSE only)

  rg::stage_attention<AP4, BLOCK>(ar_l, w_l, A.a_r, nr, A.w_alpha, A.attn_dim);
  for (int i = threadIdx.x; i < nr * AP4; i += BLOCK) gar_l[i] = rg::f4zero();
  if constexpr (RELA_LDS) {
    for (int i = threadIdx.x; i < nr * G; i += BLOCK) {
      const int r = i / G, c = i - r * G;
      rela_l[i] = c < A.ld4 ? A.rela[(int64_t)r * A.ld4 + c] : rg::f4zero();
    }
  }
  __syncthreads();
  const float b_alpha = A.b_alpha[0];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int lane_g = lane & (G - 1), gi_w = lane / G;
  float4* my_stage = stage + wv * 64 + gi_w * G;
  const bool row_lane = lane_g < A.ld4;
  const int lane_c = row_lane ? lane_g : A.ld4 - 1;

  float4 gw[AP4];
#pragma unroll
  for (int k = 0; k < AP4; ++k) gw[k] = rg::f4zero();
  float gb = 0.f;

  rg::walk_items<G, DENSE, KPG, BLOCK>(A.walk, recs, [&](const int4& R, bool live) {
    const int beg = R.x, end = R.x + rg::walk_len(R), b = R.z, s_node = R.w;
    int qt = 0, wlo = 0, whi = 0, lt = 0;
    if constexpr (L != STATIC) qt = A.q_time[b];
    if constexpr (L == WINDOWED) { wlo = A.win_lo[b]; whi = A.win_hi[b]; lt = A.loop_time[b]; }
    float4 base[AP4], gas[AP4];
#pragma unroll
    for (int k = 0; k < AP4; ++k) {
      base[k] = rg::f4add(A.a_s[(int64_t)s_node * AP4 + k], A.a_q[(int64_t)b * AP4 + k]);   // hoisted per source (attn.h)
      gas[k] = rg::f4zero();
    }
    float4 hs[ND], acc[ND];
#pragma unroll
    for (int dd = 0; dd < ND; ++dd) {
      hs[dd] = A.hidden[((int64_t)s_node * ND + dd) * A.ld4 + lane_c];
      acc[dd] = rg::f4zero();
    }
    const int2* bm_row = A.bm_new + (int64_t)b * A.W;

    for (int c0 = beg; c0 < end; c0 += G) {
      // ---- phase 1: one out-edge per lane: destination id, attention ----------------------------
      const int c = c0 + lane_g;
      bool valid = c < end;
      const int cnt = min(G, end - c0);
      int o = 0, r = 0, rrow = 0, tdir = 0;
      float alpha = 0.f;
      float4 zr[AP4];
#pragma unroll
      for (int k = 0; k < AP4; ++k) zr[k] = rg::f4zero();
      int erow = 0;
      if constexpr (L == WINDOWED) {   // an edge outside the query's window is no edge: it stays in the round as a pad (alpha = 0, row 0)
        if (valid) {
          erow = A.out_time[c];
          valid = erow >= A.n_data || (erow >= wlo && erow < whi);
        }
      }
      if (valid) {
        int tl;
        if constexpr (PACKED) { const uint32_t pk = A.out_pk[c]; tl = pk & 0xFFFFF; r = pk >> 20; }
        else { const int2 rt = A.out_rt[c]; r = rt.x; tl = rt.y; }
        o = rg::bm_rank(bm_row[tl >> 5], tl);
        rrow = r;
        if constexpr (L == WINDOWED) {
          const int delta = qt - (erow >= A.n_data ? lt : A.row_time[erow]);
          tdir = min(max(delta, 0), A.n_time - 1) * 4;
        } else if constexpr (L == TEMPORAL) {
          const int dt = A.out_time[c] - qt;
          const int dir = dt > 0 ? 2 : (dt == 0 ? 1 : 0);
          rrow = dir * nr + r;
          tdir = (dir * A.n_time + (dt < 0 ? -dt : dt)) * 4 + dir;
        }
        float z = b_alpha;
#pragma unroll
        for (int k = 0; k < AP4; ++k) rg::attn_acc(z, w_l[k], base[k], ar_l[r * AP4 + k], zr[k]);
        alpha = rg::attn_alpha(z);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();
      my_stage[lane_g] = make_float4(__int_as_float(o), __int_as_float(rrow), alpha, __int_as_float(tdir));   // pad lanes: alpha 0, row 0
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();

      // ---- phase 2: one edge per group step, U grad rows in flight --------------------------------------
      for (int k = 0; k < cnt; k += U) {
        float4 tp[U], gv[U], rv[U], tv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) tp[u] = my_stage[k + u];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          gv[u] = A.grad_agg[(int64_t)__float_as_int(tp[u].x) * A.ld4 + lane_c];
          if constexpr (L != STATIC) {
            rv[u] = A.rela[(int64_t)__float_as_int(tp[u].y) * A.ld4 + lane_c];
            tv[u] = A.time_tab[(int64_t)(__float_as_int(tp[u].w) >> 2) * A.ld4 + lane_c];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float al = tp[u].z;
          const int dir = __float_as_int(tp[u].w) & 3;
          float4 hsel = hs[0];
          if constexpr (L == TEMPORAL) hsel = dir == 0 ? hs[0] : (dir == 1 ? hs[1] : hs[2]);
          if constexpr (L == STATIC) {
            const int ru = __float_as_int(tp[u].y);
            if constexpr (RELA_LDS) rv[u] = rela_l[ru * G + lane_g];
            else rv[u] = A.rela[(int64_t)ru * A.ld4 + lane_c];
          }
          float dot = 0.f;
          if (row_lane) {
            float4 m;
            if constexpr (L == STATIC) m = make_float4(hsel.x + rv[u].x, hsel.y + rv[u].y, hsel.z + rv[u].z, hsel.w + rv[u].w);
            else m = make_float4(hsel.x + rv[u].x + tv[u].x, hsel.y + rv[u].y + tv[u].y, hsel.z + rv[u].z + tv[u].z,
                                 hsel.w + rv[u].w + tv[u].w);
            dot = gv[u].x * m.x;
            dot = fmaf(gv[u].y, m.y, dot);
            dot = fmaf(gv[u].z, m.z, dot);
            dot = fmaf(gv[u].w, m.w, dot);
          }
          dot = rg::group_sum<G>(dot);
          if (lane_g == 0) reinterpret_cast<float*>(&my_stage[k + u])[0] = dot;     // o is consumed: slot reused for g_alpha
          const float4 ag = make_float4(al * gv[u].x, al * gv[u].y, al * gv[u].z, al * gv[u].w);
          if constexpr (L == STATIC) {
            acc[0].x += ag.x; acc[0].y += ag.y; acc[0].z += ag.z; acc[0].w += ag.w;
          } else {
#pragma unroll
            for (int dd = 0; dd < ND; ++dd) {
              const float mk = (L == WINDOWED || dir == dd) ? 1.f : 0.f;
              acc[dd].x = fmaf(mk, ag.x, acc[dd].x); acc[dd].y = fmaf(mk, ag.y, acc[dd].y);
              acc[dd].z = fmaf(mk, ag.z, acc[dd].z); acc[dd].w = fmaf(mk, ag.w, acc[dd].w);
            }
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      __builtin_amdgcn_wave_barrier();

      // ---- phase 3: back to one edge per lane: attention gradients --------------------------------
      if (valid) {
        const float g_alpha = reinterpret_cast<const float*>(&my_stage[lane_g])[0];
        const float g_p = g_alpha * alpha * (1.0f - alpha);
        if constexpr (L == STATIC) gb += g_p;
#pragma unroll
        for (int k = 0; k < AP4; ++k) {
          const float4 w = w_l[k];
          gw[k].x = fmaf(g_p, zr[k].x, gw[k].x);
          gw[k].y = fmaf(g_p, zr[k].y, gw[k].y);
          gw[k].z = fmaf(g_p, zr[k].z, gw[k].z);
          gw[k].w = fmaf(g_p, zr[k].w, gw[k].w);
          const float4 gz = make_float4(zr[k].x > 0.f ? g_p * w.x : 0.f, zr[k].y > 0.f ? g_p * w.y : 0.f,
                                        zr[k].z > 0.f ? g_p * w.z : 0.f, zr[k].w > 0.f ? g_p * w.w : 0.f);
          gas[k].x += gz.x; gas[k].y += gz.y; gas[k].z += gz.z; gas[k].w += gz.w;
          float* ga = reinterpret_cast<float*>(&gar_l[r * AP4 + k]);
          if (gz.x != 0.f) atomicAdd(ga + 0, gz.x);
          if (gz.y != 0.f) atomicAdd(ga + 1, gz.y);
          if (gz.z != 0.f) atomicAdd(ga + 2, gz.z);
          if (gz.w != 0.f) atomicAdd(ga + 3, gz.w);
        }
      }
    }
    // ---- per-source (or per-segment) results -------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < AP4; ++k) {
      gas[k].x = rg::group_sum<G>(gas[k].x);
      gas[k].y = rg::group_sum<G>(gas[k].y);
      gas[k].z = rg::group_sum<G>(gas[k].z);
      gas[k].w = rg::group_sum<G>(gas[k].w);
    }
    if (live) {
      const int out = rg::walk_out(R, A.walk.n_slots);
      float4* hrow = out >= 0 ? A.g_hidden + (int64_t)out * ND * A.ld4 : A.g_hidden_part + (int64_t)(-out - 1) * ND * A.ld4;
      float4* arow = out >= 0 ? A.g_as + (int64_t)out * AP4 : A.g_as_part + (int64_t)(-out - 1) * AP4;
      if (row_lane) {
#pragma unroll
        for (int dd = 0; dd < ND; ++dd) hrow[dd * A.ld4 + lane_g] = acc[dd];
      }
      if (lane_g == 0) {
#pragma unroll
        for (int k = 0; k < AP4; ++k) arow[k] = gas[k];
      }
    }
  });

  // ---- block-level flushes ------------------------------------------------------------------------------
  __syncthreads();
  for (int i = threadIdx.x; i < nr * AP4 * 4; i += BLOCK) {
    const float v = reinterpret_cast<float*>(gar_l)[i];
    if (v != 0.f) atomicAdd(A.g_ar + i, v);
  }
  // dw (and db, STATIC): wave reduce -> LDS -> first threads
  constexpr int NV = AP4 * 4 + (L == STATIC ? 1 : 0);
  float vals[NV];
#pragma unroll
  for (int k = 0; k < AP4; ++k) { vals[4 * k] = gw[k].x; vals[4 * k + 1] = gw[k].y; vals[4 * k + 2] = gw[k].z; vals[4 * k + 3] = gw[k].w; }
  if constexpr (L == STATIC) vals[AP4 * 4] = gb;
  float* red = reinterpret_cast<float*>(red_l);
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    float v = vals[i];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) red[wv * (AP4 * 4 + 4) + i] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < NV) {
    float v = 0.f;
    for (int w = 0; w < BLOCK / 64; ++w) v += red[w * (AP4 * 4 + 4) + threadIdx.x];
    if (L == STATIC && threadIdx.x == AP4 * 4) { if (v != 0.f) atomicAdd(A.g_b, v); }
    else if ((int)threadIdx.x < A.attn_dim && v != 0.f) atomicAdd(A.g_w + threadIdx.x, v);
  }
}

// hub sources cut into segments: dH[s], dA_s[s] = sums of the segments' partial rows, in segment order (rows of cols_h + ap4 float4)
__global__ void bwd_combine_kernel(const int4* __restrict__ split, int n_split, int n_slots, int B, const int2* __restrict__ bm_old,
                                   int W, const float4* __restrict__ hpart, const float4* __restrict__ apart,
                                   float4* __restrict__ g_hidden, float4* __restrict__ g_as, int cols_h, int ap4) {
  const int cols = cols_h + ap4;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t item = tid / cols;
  const int c = (int)(tid - item * cols);
  if (item >= (int64_t)B * n_split) return;
  const int b = (int)(item / n_split);
  const int4 se = split[item - (int64_t)b * n_split];
  const int2 wp = bm_old[(int64_t)b * W + (se.x >> 5)];
  if (!rg::bm_has(wp, se.x)) return;
  const int s = rg::bm_rank(wp, se.x);
  const bool is_h = c < cols_h;
  const int stride = is_h ? cols_h : ap4;
  const float4* p = (is_h ? hpart : apart) + ((int64_t)b * n_slots + se.y) * stride + (is_h ? c : c - cols_h);
  float4 acc = p[0];
  for (int k = 1; k < se.z; ++k) {
    const float4 v = p[(int64_t)k * stride];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  if (is_h) g_hidden[(int64_t)s * cols_h + c] = acc;
  else g_as[(int64_t)s * ap4 + (c - cols_h)] = acc;
}

template <int G, int AP4, bool PACKED, bool DENSE, bool RELA_LDS, int KPG, Layer L>
int launch3(const BwdArgs& A, size_t lds, int B, const rg_vrows& vr, const int2* bm_old, hipStream_t s) {
  auto kern = layer_bwd_kernel<G, AP4, PACKED, DENSE, RELA_LDS, KPG, L>;
  if (lds > 64 * 1024) RG_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const int per_cu = lds <= 80 * 1024 ? 2 : 1;
  const int grid = rg::walk_grid(A.walk.n_items, BWD_BLOCK, G, DENSE, per_cu, KPG);
  if (rg::zero_async(A.walk.queues, RG_QUEUE_BYTES, s)) return 1;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(BWD_BLOCK), lds, s, A);
  RG_LAUNCH_CHECK();
  if (vr.n_split > 0) {
    const int cols_h = dir_rows(L) * A.ld4;
    const int64_t threads = (int64_t)B * vr.n_split * (cols_h + AP4);
    hipLaunchKernelGGL(bwd_combine_kernel, dim3(rg::ceil_div(threads, 256)), dim3(256), 0, s, vr.split, vr.n_split, vr.n_slots, B,
                       bm_old, A.W, A.g_hidden_part, A.g_as_part, A.g_hidden, A.g_as, cols_h, AP4);
    RG_LAUNCH_CHECK();
  }
  return 0;
}

template <int G, int AP4, bool PACKED, bool DENSE, Layer L>
int launch2(const char* who, const BwdArgs& A, int B, const rg_vrows& vr, const int2* bm_old, hipStream_t s) {
  size_t lds = (size_t)(BWD_BLOCK + 2 * A.n_rela_rows * AP4 + AP4 + (BWD_BLOCK / 64) * (AP4 + 1)) * sizeof(float4);
  if (!DENSE) lds += (size_t)BWD_BLOCK * sizeof(int4);
  RG_CHECK(lds <= 160 * 1024, "%s: attention tables need %zu B of LDS (> 160 KiB)", who, lds);
  if constexpr (L == STATIC) {
    // dRel comes from the relation-major pass (key_bwd_kernel.h); here the rela rows are only read
    const size_t rela = (size_t)A.n_rela_rows * G * sizeof(float4);
    const bool rela_lds = lds + rela <= 80 * 1024;
    if constexpr (DENSE) {
      if (A.kpg > 1) {
        if (rela_lds) return launch3<G, AP4, PACKED, true, true, rg::RG_KPG_SHORT, L>(A, lds + rela + 64, B, vr, bm_old, s);
        return launch3<G, AP4, PACKED, true, false, rg::RG_KPG_SHORT, L>(A, lds, B, vr, bm_old, s);
      }
    }
    if (rela_lds) return launch3<G, AP4, PACKED, DENSE, true, 1, L>(A, lds + rela + 64, B, vr, bm_old, s);
    return launch3<G, AP4, PACKED, DENSE, false, 1, L>(A, lds, B, vr, bm_old, s);
  } else {
    return launch3<G, AP4, false, DENSE, false, 1, L>(A, lds, B, vr, bm_old, s);
  }
}

// the layer kernel (and the combine kernel for cut sources) at the widths ld4 = A.ld4, ap4; dense: the dense walk
template <Layer L>
int launch(const char* who, const BwdArgs& A, int ap4, int B, const rg_vrows& vr, const int2* bm_old, bool dense, hipStream_t s) {
  return rg::with_g(A.ld4, [&](auto g) {
    return rg::with_ap4(ap4, who, [&](auto ap) {
      constexpr int G = decltype(g)::value, AP4 = decltype(ap)::value;
      if constexpr (L == STATIC) {
        if (A.out_pk) return dense ? launch2<G, AP4, true, true, L>(who, A, B, vr, bm_old, s) : launch2<G, AP4, true, false, L>(who, A, B, vr, bm_old, s);
      }
      return dense ? launch2<G, AP4, false, true, L>(who, A, B, vr, bm_old, s) : launch2<G, AP4, false, false, L>(who, A, B, vr, bm_old, s);
    });
  });
}

// checks shared by the static and the temporal entry points; need: the entry point's scratch bytes
inline int check_common(const char* who, const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, int32_t d, int32_t ld,
                        int32_t ap, int32_t attn_dim, const void* scratch, size_t scratch_bytes, size_t need) {
  RG_CHECK(g->n_ent == f->n_ent, "%s: graph has %d entities, frontier %d", who, g->n_ent, f->n_ent);
  RG_CHECK(level >= 1 && level <= f->level && level > f->level - f->n_levels + 1,
           "%s: level %d not resident (current %d, %d kept)", who, level, f->level, f->n_levels);
  RG_CHECK(n_old == f->n_nodes[(level - 1) % f->n_levels], "%s: n_old=%lld but level %d has %lld nodes", who,
           (long long)n_old, level - 1, (long long)f->n_nodes[(level - 1) % f->n_levels]);
  RG_CHECK(d > 0 && ld >= d && ld % 4 == 0 && ld >= 16 && ld <= 256, "%s: d=%d ld=%d", who, d, ld);
  RG_CHECK(attn_dim > 0 && ap >= attn_dim && ap % 4 == 0, "%s: attn_dim=%d ap=%d", who, attn_dim, ap);
  RG_CHECK(g->out_vr.n_slots == 0 || (scratch && scratch_bytes >= need), "%s: scratch %zu B < required %zu B", who,
           scratch_bytes, need);
  RG_CHECK((int64_t)f->B * std::max(g->out_vr.n_slots, 1) < ((int64_t)1 << 31) && g->out_vr.n_slots < (1 << 22),
           "%s: batch * hub segments overflows int32", who);
  const int64_t n_items = (int64_t)f->B * g->out_vr.n;
  RG_CHECK(n_items / 8 + ((int64_t)1 << 26) < ((int64_t)1 << 31), "%s: work space too large for 32-bit queue tickets", who);
  return 0;
}

// the walk over level - 1's sources and the scratch layout: partial rows of cut sources [B * n_slots][nd * ld], then their dA_s
inline void fill_common(const rg_frontier* f, const rg_graph* g, int32_t level, int32_t ld, int nd, void* scratch, BwdArgs* A) {
  A->walk.n_items = (int64_t)f->B * g->out_vr.n; A->walk.n_vrows = g->out_vr.n; A->walk.n_slots = g->out_vr.n_slots;
  A->walk.vrows = g->out_vr.rows; A->walk.bm_test = f->bm_of(level - 1); A->walk.W = f->W; A->walk.queues = f->queues;
  f->queues_clean = false;
  A->out_rt = g->out_rt;
  A->bm_new = f->bm_of(level); A->W = f->W;
  A->ld4 = ld / 4; A->n_rela_rows = g->n_rela_rows;
  A->g_hidden_part = (float4*)scratch;
  A->g_as_part = (float4*)((char*)scratch + rg::align_up((size_t)f->B * g->out_vr.n_slots * nd * ld * sizeof(float), 256));
}

}  // namespace
}  // namespace rgbwd
