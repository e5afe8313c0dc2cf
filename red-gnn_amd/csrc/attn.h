// Device pieces every kernel that evaluates an edge's attention is made of: the frontier-bitmap lookup, the attention scalar
//   alpha = sigmoid(w . relu(a_s[s] + a_r[r] + a_q[b]) + b_alpha)
// and the per-group compaction of a round's surviving candidates.  The only definition of each: the layer forward
// (layer_fwd_kernel.h, layer_fwd_wp.hip), its adjoint (layer_bwd_kernel.h, key_bwd_kernel.h), explain.hip and profile.hip call these.
//
// Order of the three-term sum.  attn_acc adds TWO operands; the caller forms the pair, and the pair it forms is its contract:
//   (a_s + a_r) + a_q   attn_acc_fwd, the forward family: layer_fwd_kernel, layer_fwd_wp_kernel, explain_kernel, profile_kernel,
//                       and the temporal / windowed key-major passes.  This is the order "the forward's alpha bit for bit" refers
//                       to: explain and profile threshold and sum the very float the forward multiplied by.
//   (a_s + a_q) + a_r   attn_acc(base, a_r) in layer_bwd_kernel: a hoist, a_s[s] + a_q[b] is constant over a source's out-edges.
//   a_s + (a_r + a_q)   attn_acc(a_s, base) in the static key-major pass: a hoist, a_r[r] + a_q[b] is constant over an item (one
//                       relation, one query).
// The two hoisted orders differ from the forward's by a rounding of the pre-activation; the adjoint is checked against the
// forward to a tolerance, never bit for bit, so they stay hoisted.
#pragma once
#include "common.h"

namespace rg {

// ---- frontier bitmaps: wp = {word, exclusive popcount prefix} of entity e's word (common.h rg_frontier) ------------------
__device__ __forceinline__ bool bm_has(const int2& wp, int e) { return ((uint32_t)wp.x >> (e & 31)) & 1u; }
// node id of e in its level (meaningful where bm_has)
__device__ __forceinline__ int bm_rank(const int2& wp, int e) { return wp.y + __popc((uint32_t)wp.x & ((1u << (e & 31)) - 1u)); }

// ---- attention scalar ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 f4add(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// components 4k .. 4k+3 of w_alpha, zero from attn_dim on (the tables are padded to a multiple of four columns)
__device__ __forceinline__ float4 attn_w4(const float* __restrict__ w_alpha, int attn_dim, int k) {
  float w[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) w[u] = 4 * k + u < attn_dim ? w_alpha[4 * k + u] : 0.f;
  return make_float4(w[0], w[1], w[2], w[3]);
}

// LDS prologue: ar_l [n_rows][AP4] = a_r, w_l [AP4] = masked w_alpha.  The caller's __syncthreads() follows.
template <int AP4, int BLOCK>
__device__ __forceinline__ void stage_attention(float4* ar_l, float4* w_l, const float4* __restrict__ a_r, int n_rows,
                                                const float* __restrict__ w_alpha, int attn_dim) {
  for (int i = threadIdx.x; i < n_rows * AP4; i += BLOCK) ar_l[i] = a_r[i];
  if (threadIdx.x < AP4) w_l[threadIdx.x] = attn_w4(w_alpha, attn_dim, threadIdx.x);
}

// one component: z += w * zr,  zr = relu(pre); returns zr
__device__ __forceinline__ float attn_term(float& z, float w, float pre) {
  const float zr = fmaxf(pre, 0.f);
  z = fmaf(w, zr, z);
  return zr;
}
// z += w . zr,  zr = relu(u + v): four fmas in x, y, z, w order, each component's sum formed right before its fma
__device__ __forceinline__ void attn_acc(float& z, const float4& w, const float4& u, const float4& v, float4& zr) {
  zr.x = attn_term(z, w.x, u.x + v.x);
  zr.y = attn_term(z, w.y, u.y + v.y);
  zr.z = attn_term(z, w.z, u.z + v.z);
  zr.w = attn_term(z, w.w, u.w + v.w);
}
__device__ __forceinline__ void attn_acc(float& z, const float4& w, const float4& u, const float4& v) {
  float4 zr;
  attn_acc(z, w, u, v, zr);
}
// the forward's pair, (a_s + a_r, a_q), formed inside: attn_acc(z, w, f4add(as, ar), aq) is the same arithmetic but puts the four
// a_s + a_r ahead of the first fma, and from that order the compiler spills in the word-parallel and the 80-register forward kernels
__device__ __forceinline__ void attn_acc_fwd(float& z, const float4& w, const float4& as, const float4& ar, const float4& aq) {
  attn_term(z, w.x, as.x + ar.x + aq.x);
  attn_term(z, w.y, as.y + ar.y + aq.y);
  attn_term(z, w.z, as.z + ar.z + aq.z);
  attn_term(z, w.w, as.w + ar.w + aq.w);
}

__device__ __forceinline__ float attn_alpha(float z) { return __builtin_amdgcn_rcpf(1.0f + __expf(-z)); }

// ---- compaction of a round's candidates ------------------------------------------------------------------------------------
// Every group of G lanes owns a strip of G tuples: the lanes with `valid` store t at their rank among the group's valid lanes, the
// slots from the count on are zeroed (pad tuples: alpha 0, row 0); returns the count.  The fences order the strip's previous
// readers before the stores and the stores before the next readers.  WG_RELEASE picks the fence and is part of each kernel's
// tuning, not a detail to unify: release at workgroup scope in the backward passes, acq_rel at wavefront scope in the forward.
template <bool WG_RELEASE>
__device__ __forceinline__ void strip_fence() {
  if constexpr (WG_RELEASE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  else __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

template <int G, bool WG_RELEASE>
__device__ __forceinline__ int group_compact(float4* my_stage, int lane, bool valid, const float4& t) {
  const int lane_g = lane & (G - 1), gshift = lane & ~(G - 1);
  const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
  const unsigned long long m = (__ballot(valid) >> gshift) & gmask;
  const int cnt = __popcll(m);
  const int pos = __popcll(m & ((1ull << lane_g) - 1ull));
  strip_fence<WG_RELEASE>();
  if (lane_g >= cnt) my_stage[lane_g] = f4zero();
  if (valid) my_stage[pos] = t;
  strip_fence<WG_RELEASE>();
  return cnt;
}

}  // namespace rg
