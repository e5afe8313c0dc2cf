// Shared by the six fused dense kernels (dense.hip, dense_split.hip, dense_split3.hip: d <= 64 with the weights resident in LDS;
// dense128.hip, dense128_split.hip, dense128_split3.hip: d = 128 with the weights streamed through LDS) and by dense_bwd.hip:
// the argument block and its filler, the grid and the activation dispatch of the launchers, compile-time helpers, and device code
// around the tile loops (abs-max scan of a weight matrix, row maximum, GRU bias table, slot swizzle of the f16 weight images).
// The f16 split arithmetic is in split3.h.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>
#include "common.h"

namespace rg {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// threads per workgroup of the d <= 64 kernels: 8 waves (2 per SIMD, <= 256 VGPRs)
constexpr int DENSE_T = 512;
constexpr float LOG2E = 1.44269504088896340736f;

struct DenseArgs {
  int64_t n = 0;                     // number of node rows, or their capacity when n_dev is given
  const int32_t* n_dev = nullptr;    // device-side count (after rg_frontier_expand_async), or null
  int d = 0, ld4 = 0;                // true width, row stride in float4
  const float4* agg = nullptr;
  const float4* hprev = nullptr;     // [n_old][ld4]
  const int32_t* prev_idx = nullptr; // [n] or null (all new)
  const float* W_h = nullptr;        // [d][d]
  const float* w_ih = nullptr;       // [3d][d]
  const float* w_hh = nullptr;
  const float* b_ih = nullptr;       // [3d]
  const float* b_hh = nullptr;
  const float* Ws = nullptr;         // [attn][d] or null
  int attn = 0, ap = 0;
  float* a_s_out = nullptr;          // [n][ap]
  const float* W_final = nullptr;    // [d] or null
  const int32_t* nodes = nullptr;    // [n][2]
  int n_ent = 0;
  float* scores = nullptr;           // [B*n_ent]
  float4* hidden_out = nullptr;      // [n][ld4]
  int act = 0;                       // 0 idd, 1 relu, 2 tanh
  int n_tiles = 0;
  int64_t n_hint = 0;      // host side: expected number of rows when n is only a capacity (sizes the grid; any value is correct)
  // training variant (rg_dense_train_fwd): dropout mask in, GRU input and gate workspace out
  const float* mask = nullptr;   // [n][ld] 0 or 1/(1-p), or null
  float* x_out = nullptr;        // [n][ld]  act(W_h agg) * mask
  int probe = 0;                 // three-term kernel, test hook (rg_split3_product_check): 1 = hidden_out <- act(W_h agg), 2 = W_in x, 3 = W_hn h
  float* ws_out = nullptr;       // [n][5][d] = {r, z, n, h0, W_hn h0 + b_hn}: the workspace layout of aten's fused GRU cell
};

// The operands every launch has; what a caller does not set afterwards (device-side count, projection, readout, training outputs,
// probe) stays off.
inline DenseArgs dense_args(int64_t n, int d, int ld, const float* agg, const float* hidden_prev, const int32_t* prev_idx, const float* W_h,
                            int act, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, float* hidden_out) {
  DenseArgs A;
  A.n = n; A.d = d; A.ld4 = ld / 4;
  A.agg = (const float4*)agg; A.hprev = (const float4*)hidden_prev; A.prev_idx = prev_idx;
  A.W_h = W_h; A.w_ih = w_ih; A.w_hh = w_hh; A.b_ih = b_ih; A.b_hh = b_hh;
  A.hidden_out = (float4*)hidden_out; A.act = act;
  A.n_tiles = (int)ceil_div(n, 16);
  return A;
}

// Grid of a launch whose workgroups take one 16-row tile per wave and pass: one persistent workgroup per CU at most; with a
// device-side row count the grid follows the caller's expectation (+25 %) instead of the capacity: a 50-query batch has a few hundred
// tiles, and 256 workgroups staging 123 KB of weights each kept every CU busy for 30 us per launch while other streams' batches waited
inline int dense_grid(const DenseArgs& A, int waves_per_group) {
  const int64_t tiles = A.n_dev && A.n_hint > 0 ? std::min<int64_t>(A.n_tiles, ceil_div(A.n_hint + A.n_hint / 4, 16)) : A.n_tiles;
  return (int)std::max<int64_t>(std::min<int64_t>(ceil_div(tiles, waves_per_group), 256), 1);
}

// f(std::integral_constant<int, ACT>()) for the activation of the launch (the split kernels take it at compile time)
template <typename F>
inline int with_act(int act, F&& f) {
  return act == 0 ? f(std::integral_constant<int, 0>()) : act == 1 ? f(std::integral_constant<int, 1>()) : f(std::integral_constant<int, 2>());
}

// v_exp_f32 / v_rcp_f32 forms (1 ulp each; __builtin_amdgcn_rcpf, not the correctly rounded __frcp_rn which expands
// to a full division): far inside the 1e-4 relative tolerance of the path
static __device__ __forceinline__ float fast_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
static __device__ __forceinline__ float fast_tanh(float x) {
  const float e = __expf(-2.0f * fabsf(x));            // in (0, 1]: no overflow
  return copysignf((1.0f - e) * __builtin_amdgcn_rcpf(1.0f + e), x);
}

// ---- compile-time helpers of the pipelined gate loops (dense_split3.hip, dense128_split3.hip) ---------------------------------------
// an empty volatile asm that consumes and redefines a register: volatile asms keep their order, so the instruction that produced the value
// stays ahead of it and its users stay behind it - the pipelined gate loops fix their instruction order with these
#define RG_PIN(x) asm volatile("" : "+v"(x))
#define RG_PIN_ACC(x) asm volatile("" : "+a"(x))  // the same for an MFMA accumulator that lives in the accumulation registers

template <class Fn, int... I>
__device__ __forceinline__ void static_for_impl(Fn&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class Fn>
__device__ __forceinline__ void static_for(Fn&& f) { static_for_impl(f, std::make_integer_sequence<int, N>{}); }

// ---- device code around the tile loops ------------------------------------------------------------------------------------------------
// wm = max(wm, largest magnitude of the n4 float4 at src) over the strides of this thread in a workgroup of T; a matrix that is not
// there has none
template <int T>
__device__ __forceinline__ void abs_max_scan(float& wm, const float* src, int n4) {
  if (!src) return;
  for (int i = threadIdx.x; i < n4; i += T) {
    const float4 q = reinterpret_cast<const float4*>(src)[i];
    wm = fmaxf(fmaxf(wm, fmaxf(fabsf(q.x), fabsf(q.y))), fmaxf(fabsf(q.z), fabsf(q.w)));
  }
}

// max(m, largest magnitude of the lane's node row): the row is spread over the four lane quarters
template <int KS>
__device__ __forceinline__ float row_abs_max(const float (&f)[KS], float m) {
#pragma unroll
  for (int i = 0; i < KS; ++i) m = fmaxf(m, fabsf(f[i]));
  m = fmaxf(m, __shfl_xor(m, 16));
  m = fmaxf(m, __shfl_xor(m, 32));
  return m;
}

// GRU bias table [4][DP] of a workgroup of T threads: b_ir + b_hr, b_iz + b_hz, b_in, b_hn.  FOLDED: pre-multiplied by the exp2 factors
// of their gates (sigmoid(a) = 1 / (1 + 2^(-log2e a)), tanh(a) = 2 / (1 + 2^(-2 log2e a)) - 1).  PAD: the true width d is below DP
// and columns beyond it are zero; otherwise d = DP.
template <int T, int DP, bool FOLDED, bool PAD>
__device__ __forceinline__ void fill_gru_bias(float* bias_l, const DenseArgs& A, int d) {
  constexpr float fs = FOLDED ? -LOG2E : 1.0f, ft = FOLDED ? -2.0f * LOG2E : 1.0f;
  for (int i = threadIdx.x; i < 4 * DP; i += T) {
    const int g = i / DP, c = i - g * DP;
    float v = 0.f;
    if (!PAD || c < d) {
      if (g == 0) v = fs * (A.b_ih[c] + A.b_hh[c]);
      else if (g == 1) v = fs * (A.b_ih[d + c] + A.b_hh[d + c]);
      else if (g == 2) v = ft * A.b_ih[2 * d + c];
      else v = ft * A.b_hh[2 * d + c];
    }
    bias_l[i] = v;
  }
}

// ---- f16 weight images of the d <= 64 split kernels -------------------------------------------------------------------------------------
// DP in {32, 64}: padded width.  Per row DP f16 values of a part (hi, and in a second image lo or mid); the 16-B slot (k-step s, lane
// quarter hq) holds the row's weights for k = 16 * (2s + j / 4) + 4 * hq + j % 4, j = 0..7 - the k order in which a lane holds its
// accumulator rows, so that accumulators convert in place into the next B fragment.  Slots are XOR-swizzled with the row so that the
// 16 rows read by a quarter wave cover the 16 bank groups.  The three-term kernel's bf8 lo image has the same slots at 8 B each, swizzled
// so that the one read per product that fetches all its k-steps is free of bank conflicts.
template <int DP>
struct Geo {
  static constexpr int SR = DP / 8;                  // slots per image row
  static constexpr int SH = DP == 64 ? 1 : 2;        // rows per 256 B of the f16 images
  static constexpr int KST = DP / 32;                // k-steps of 32 per product
  __device__ static __forceinline__ int at(int row, int slot) { return row * SR + (slot ^ ((row >> SH) & (SR - 1))); }
  // bf8 lo image, byte offset of the lane quarter hq's values of a row: DP = 64: 16 B = {k-step 0, k-step 1} (one ds_read_b128 per
  // product; its 4 x 16 lane groups {0-3, 12-15, 20-27}, ... then cover the 64 banks: slot = hq ^ f(row / 4), f = 0, 3, 2, 1);
  // DP = 32: 8 B (one k-step), slot = hq ^ 2 (row / 8)
  __device__ static __forceinline__ int at8(int row, int hq) {
    if (DP == 64) {
      const int g = (row >> 2) & 3, f = (4 - g) & 3;
      return row * 64 + ((hq ^ f) << 4);
    }
    return row * 32 + ((hq ^ (((row >> 3) & 1) << 1)) << 3);
  }
};

// d = 128 (dense128.hip)
int dense128_launch(const DenseArgs& A, hipStream_t s);
// d <= 64 with the products as two-term f16 splits (dense_split.hip)
int dense_split_launch(const DenseArgs& A, hipStream_t s);
// d <= 64 with the products as exact three-term f16 splits = fp32 arithmetic on the f16 pipe (dense_split3.hip)
int dense_split3_launch(const DenseArgs& A, hipStream_t s);
// d = 128 with exact three-term splits, weights streamed from a split image in a caller-provided scratch (dense128_split3.hip)
int64_t dense128_split3_scratch_bytes();
int dense128_split3_launch(const DenseArgs& A, void* scratch, int64_t scratch_bytes, hipStream_t s);
// d = 128 with split products: the weights' split image goes through a caller-provided scratch (dense128_split.hip)
int64_t dense128_split_scratch_bytes();
int dense128_split_launch(const DenseArgs& A, void* scratch, int64_t scratch_bytes, hipStream_t s);

}  // namespace rg
