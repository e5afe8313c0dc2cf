// out[r, :n] = x[r, :k] W^T (+ bias) for node-row matrices, W [n][k] as torch keeps a linear's weight: a row's result does not depend
// on how many rows the call has.
//
// The extrapolation model's inference forward (extrapolation.py, T_RED_GNN._run) forms its per-row products - the attention inputs a_s
// and a_q, the hoisted W_past products, the time table, the classifier - with this kernel instead of a GEMM library call.  A library
// picks its kernel, and with it the order of a dot product's additions, by the number of rows, so the same query got other last bits
// in a batch of 1 than in a batch of 33; here every output element is one thread's fmaf chain over k = 0, 1, ..., k - 1, whatever the
// row count, the grid or the column tile.  That is what makes the integer tables of attention_profile equal across splits of a batch.
//
// Mapping: one thread per (row, four consecutive output columns); W^T staged in LDS as [k][nc] (nc a multiple of 4, zero-padded past
// n), read as float4 along the columns - the lanes of a row read consecutive float4; the x row is read by the nc / 4 threads of the
// row (float4 loads where k, the row stride and the base allow, scalar loads otherwise: the same chain).  Columns are tiled on the host
// so that a tile's weights fit 64 KB of LDS.  The products are small against the layer kernels (N rows x k x n fmaf, rows read once
// from HBM and nc / 4 times from L1); not measured alone.
#include <algorithm>

#include "common.h"

namespace {

constexpr int RL_BLOCK = 256;
constexpr size_t RL_LDS_MAX = 64 * 1024;

template <bool VEC>
__global__ __launch_bounds__(RL_BLOCK) void rows_linear_kernel(const float* __restrict__ x, int64_t n_rows, int64_t ldx, int k,
                                                               const float* __restrict__ w, const float* __restrict__ bias, int n, int c0,
                                                               int nc4, float* __restrict__ out, int64_t ldo) {
  extern __shared__ __align__(16) unsigned char rl_smem[];
  float* w_l = (float*)rl_smem;                         // [k][nc4 * 4]: w_l[j][c] = W[c0 + c][j], 0 past n
  const int nc = nc4 * 4;
  for (int i = threadIdx.x; i < k * nc; i += RL_BLOCK) {
    const int j = i / nc, c = i - j * nc;
    w_l[i] = c0 + c < n ? w[(int64_t)(c0 + c) * k + j] : 0.f;
  }
  __syncthreads();
  const float4* w4 = (const float4*)w_l;
  const int64_t total = n_rows * nc4;
  for (int64_t t = (int64_t)blockIdx.x * RL_BLOCK + threadIdx.x; t < total; t += (int64_t)gridDim.x * RL_BLOCK) {
    const int64_t r = t / nc4;
    const int c = (int)(t - r * nc4);
    const float* xr = x + r * ldx;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (VEC) {
      for (int j = 0; j < k; j += 4) {
        const float4 xv = *reinterpret_cast<const float4*>(xr + j);
        const float xs[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float4 wv = w4[(j + u) * nc4 + c];
          acc.x = fmaf(xs[u], wv.x, acc.x); acc.y = fmaf(xs[u], wv.y, acc.y); acc.z = fmaf(xs[u], wv.z, acc.z); acc.w = fmaf(xs[u], wv.w, acc.w);
        }
      }
    } else {
      for (int j = 0; j < k; ++j) {
        const float xj = xr[j];
        const float4 wv = w4[j * nc4 + c];
        acc.x = fmaf(xj, wv.x, acc.x); acc.y = fmaf(xj, wv.y, acc.y); acc.z = fmaf(xj, wv.z, acc.z); acc.w = fmaf(xj, wv.w, acc.w);
      }
    }
    const int col = c0 + 4 * c;
    const float a[4] = {acc.x, acc.y, acc.z, acc.w};
    float* o = out + r * ldo;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (col + u < n) o[col + u] = bias ? a[u] + bias[col + u] : a[u];
  }
}

}  // namespace

extern "C" int rg_rows_linear(const float* x, int64_t n_rows, int64_t ldx, int32_t k, const float* w, const float* bias, int32_t n,
                              float* out, int64_t ldo, void* stream) {
  RG_CHECK(n_rows >= 0 && k >= 1 && k <= 4096 && n >= 1, "rg_rows_linear: n_rows=%lld k=%d (1..4096) n=%d", (long long)n_rows, k, n);
  if (n_rows == 0) return 0;
  RG_CHECK(x && w && out, "rg_rows_linear: NULL argument");
  RG_CHECK(ldx >= k && ldo >= n, "rg_rows_linear: ldx=%lld < k=%d or ldo=%lld < n=%d", (long long)ldx, k, (long long)ldo, n);
  RG_CHECK(n_rows <= ((int64_t)1 << 40), "rg_rows_linear: n_rows=%lld too large", (long long)n_rows);
  // column tile: all columns where W^T fits 64 KB of LDS, else as many float4 columns as fit (k <= 4096: at least one)
  const int n4 = (n + 3) / 4;
  const int fit4 = (int)std::max<size_t>(RL_LDS_MAX / ((size_t)k * 16), 1);
  const int tile4 = std::min(n4, fit4);
  const bool vec = k % 4 == 0 && ldx % 4 == 0 && ((uintptr_t)x & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  for (int c4 = 0; c4 < n4; c4 += tile4) {
    const int nc4 = std::min(tile4, n4 - c4);
    const size_t smem = (size_t)k * nc4 * 16;
    const int grid = (int)std::max<int64_t>(std::min<int64_t>(rg::ceil_div(n_rows * nc4, RL_BLOCK), 256 * 16), 1);
    if (vec) hipLaunchKernelGGL(rows_linear_kernel<true>, dim3(grid), dim3(RL_BLOCK), smem, s, x, n_rows, ldx, k, w, bias, n, c4 * 4, nc4, out, ldo);
    else hipLaunchKernelGGL(rows_linear_kernel<false>, dim3(grid), dim3(RL_BLOCK), smem, s, x, n_rows, ldx, k, w, bias, n, c4 * 4, nc4, out, ldo);
    RG_LAUNCH_CHECK();
  }
  return 0;
}
