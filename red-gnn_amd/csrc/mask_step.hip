// One step of learning an edge mask on an r-digraph (rg_mask_step): the executor behind explain.RDigraph.learn_mask, once per
// iteration for all replicas.  A replica k holds a logit theta per edge, the gate g = sigmoid(theta) that rg_digraph_layer_fwd_gates
// multiplies the edge's message by, and Adam's two moments; the caller has run the gated forward and its adjoint at the current
// gates and hands over the scores and grad = d score / d gate.  Per replica k and row b the objective is
//
//   L[k, b] = ((score - target) * inv_scale)^2  +  lambda_size[k] * inv_n[b] * sum_e g_e  +  lambda_ent[k] * sum_e H(g_e)
//
// H the binary entropy, dH/dg = -theta exactly.  For every FREE edge e of row b:
//
//   g     = 1 / (1 + expf(-theta))
//   coef  = 2 (score[k, b] - target[b]) inv_scale[b]^2
//   dL/dg = coef * grad[k, e] + lambda_size[k] * inv_n[b] - lambda_ent[k] * theta
//   gt    = dL/dg * g (1 - g)
//   m'    = beta1 m + (1 - beta1) gt          v' = beta2 v + (1 - beta2) gt^2
//   theta'= theta - lr * (m' / (1 - beta1^t)) / (sqrtf(v' / (1 - beta2^t)) + eps)
//   gate_out = 1 / (1 + expf(-theta'))
//
// and an edge that is not free keeps theta, m, v and gate_out: nothing is stored there.  Two statistics per (replica, row) over the
// row's free edges: size_out = sum of gate_out, count_out = how many have gate_out > 0.5.
//
// Mapping (wave64): the edges of a digraph are ordered by row, so a (replica, row) pair is the contiguous range offsets[b] ..
// offsets[b + 1] of the replica's arrays, and it is owned by one wave.  The kernel is memory-bound (five arrays read, four written per
// cell, nothing reused), so a lane takes four consecutive edges with one 16-byte access per array where all four are inside the row
// (the range starts wherever the row does: the accesses are dword-aligned, which global memory takes), and two such groups per pass,
// eight loads in flight per array.  A group with an edge that is not free, or the row's last partial group, stores per element.
//
// The sum (the project's split rule): a row is cut into chunks of MASK_CHUNK edges counted from ITS OWN first edge.  Inside a chunk
// lane j adds its eight gates in edge order and the lanes are added by a butterfly; the chunk sums are added in chunk order.  No float
// atomics and no dependence on where the row lies or on the other replicas: every output has the same bits on every run, and replica
// k's are those of an n_rep = 1 call.
#include "common.h"

namespace rgms {
namespace {

constexpr int MASK_CHUNK = RG_MASK_CHUNK;         // edges per chunk of a row (include/redgnn.h): 64 lanes x 2 groups of 4
constexpr int MS_BLOCK = 256;                     // 4 waves, a (replica, row) pair each
static_assert(MASK_CHUNK == 512, "a pass of the wave is two float4 groups per lane");

struct __attribute__((aligned(4))) f4u { float x, y, z, w; };        // a 16-byte access that is only dword-aligned
struct __attribute__((aligned(1))) b4u { uint8_t x, y, z, w; };

struct MsArgs {
  int n_rep, B;
  int64_t E;
  const int64_t* offsets;
  const uint8_t* free_edge;
  const float* score;
  const float* target;
  const float* inv_scale;
  const float* inv_n;
  const float* lambda_size;
  const float* lambda_ent;
  const float* grad;
  float lr, beta1, beta2, eps, bc1, bc2;
  float* theta;
  float* m;
  float* v;
  float* gate_out;
  float* size_out;
  int32_t* count_out;
};

struct Hyper { float coef, size_term, l_ent, lr, beta1, beta2, eps, bc1, bc2; };

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// one cell: the new (theta, m, v) in place and the new gate
__device__ __forceinline__ float cell(const Hyper& H, float grad, float& theta, float& m, float& v) {
  const float g = sigmoidf(theta);
  const float dl = H.coef * grad + H.size_term - H.l_ent * theta;
  const float gt = dl * (g * (1.f - g));
  m = H.beta1 * m + (1.f - H.beta1) * gt;
  v = H.beta2 * v + (1.f - H.beta2) * (gt * gt);
  theta = theta - H.lr * (m / H.bc1) / (sqrtf(v / H.bc2) + H.eps);
  return sigmoidf(theta);
}

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__global__ __launch_bounds__(MS_BLOCK) void mask_step_kernel(MsArgs A) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * (MS_BLOCK / 64) + (threadIdx.x >> 6);
  if (item >= (int64_t)A.n_rep * A.B) return;            // (a whole wave: the exchanges below never read an inactive lane)
  const int k = (int)(item / A.B), b = (int)(item - (int64_t)k * A.B);
  const int64_t lo = min(max(A.offsets[b], (int64_t)0), A.E);
  const int64_t hi = max(min(max(A.offsets[b + 1], (int64_t)0), A.E), lo);
  Hyper H;
  {
    const float is = A.inv_scale[b];
    H.coef = 2.f * (A.score[item] - A.target[b]) * is * is;
    H.size_term = A.lambda_size[k] * A.inv_n[b];
    H.l_ent = A.lambda_ent[k];
    H.lr = A.lr; H.beta1 = A.beta1; H.beta2 = A.beta2; H.eps = A.eps; H.bc1 = A.bc1; H.bc2 = A.bc2;
  }
  const int64_t base = (int64_t)k * A.E;                 // the replica's arrays
  const float* grad = A.grad + base;
  float* theta = A.theta + base;
  float* mom = A.m + base;
  float* var = A.v + base;
  float* gate = A.gate_out + base;

  float size = 0.f;
  int count = 0;
  for (int64_t c0 = lo; c0 < hi; c0 += MASK_CHUNK) {     // (wave-uniform)
    float part = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int64_t e0 = c0 + u * 256 + lane * 4;
      const int n = (int)min(max(hi - e0, (int64_t)0), (int64_t)4);
      if (n == 4) {
        const b4u f = *(const b4u*)(A.free_edge + e0);
        const bool fr[4] = {f.x != 0, f.y != 0, f.z != 0, f.w != 0};
        if (fr[0] | fr[1] | fr[2] | fr[3]) {
          const f4u gr = *(const f4u*)(grad + e0);
          f4u th = *(const f4u*)(theta + e0), mm = *(const f4u*)(mom + e0), vv = *(const f4u*)(var + e0);
          float g[4];
          g[0] = cell(H, gr.x, th.x, mm.x, vv.x);
          g[1] = cell(H, gr.y, th.y, mm.y, vv.y);
          g[2] = cell(H, gr.z, th.z, mm.z, vv.z);
          g[3] = cell(H, gr.w, th.w, mm.w, vv.w);
          if (fr[0] & fr[1] & fr[2] & fr[3]) {
            *(f4u*)(theta + e0) = th; *(f4u*)(mom + e0) = mm; *(f4u*)(var + e0) = vv;
            *(f4u*)(gate + e0) = f4u{g[0], g[1], g[2], g[3]};
          } else {
            const float t4[4] = {th.x, th.y, th.z, th.w}, m4[4] = {mm.x, mm.y, mm.z, mm.w}, v4[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (fr[i]) { theta[e0 + i] = t4[i]; mom[e0 + i] = m4[i]; var[e0 + i] = v4[i]; gate[e0 + i] = g[i]; }
          }
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (fr[i]) { part += g[i]; count += g[i] > 0.5f; }
        }
      } else {
        for (int i = 0; i < n; ++i) {                    // the row's last, partial group
          const int64_t e = e0 + i;
          if (!A.free_edge[e]) continue;
          float th = theta[e], mm = mom[e], vv = var[e];
          const float g = cell(H, grad[e], th, mm, vv);
          theta[e] = th; mom[e] = mm; var[e] = vv; gate[e] = g;
          part += g; count += g > 0.5f;
        }
      }
    }
    size += wave_sum(part);                              // the chunk's sum, then the chunks in chunk order
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o, 64);
  if (lane == 0) { A.size_out[item] = size; A.count_out[item] = count; }
}

}  // namespace
}  // namespace rgms

extern "C" int rg_mask_step(int32_t n_rep, int32_t batch, int64_t n_edges, const int64_t* offsets, const uint8_t* free_edge,
                            const float* score, const float* target, const float* inv_scale, const float* inv_n,
                            const float* lambda_size, const float* lambda_ent, const float* grad, float lr, float beta1, float beta2,
                            float eps, int32_t step, float* theta, float* m, float* v, float* gate_out, float* size_out,
                            int32_t* count_out, void* stream) {
  const char* who = "rg_mask_step";
  RG_CHECK(n_rep >= 1, "%s: n_rep=%d (need at least one replica)", who, n_rep);
  RG_CHECK(step >= 1, "%s: step=%d (steps count from 1)", who, step);
  RG_CHECK(batch >= 0 && n_edges >= 0, "%s: batch=%d n_edges=%lld (negative size)", who, batch, (long long)n_edges);
  RG_CHECK(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: beta1=%g beta2=%g (need 0 <= beta < 1)", who, (double)beta1,
           (double)beta2);
  RG_CHECK((int64_t)n_rep * n_edges < ((int64_t)1 << 31) && (int64_t)n_rep * batch < ((int64_t)1 << 31),
           "%s: n_rep=%d times n_edges=%lld or batch=%d overflows int32", who, n_rep, (long long)n_edges, batch);
  RG_CHECK(offsets && free_edge && score && target && inv_scale && inv_n && lambda_size && lambda_ent && grad && theta && m && v &&
           gate_out && size_out && count_out, "%s: NULL argument", who);
  if (n_edges == 0 || batch == 0) return 0;              // nothing to update and nothing launched: the caller owns the outputs
  rgms::MsArgs A;
  A.n_rep = n_rep; A.B = batch; A.E = n_edges; A.offsets = offsets; A.free_edge = free_edge;
  A.score = score; A.target = target; A.inv_scale = inv_scale; A.inv_n = inv_n; A.lambda_size = lambda_size; A.lambda_ent = lambda_ent;
  A.grad = grad; A.lr = lr; A.beta1 = beta1; A.beta2 = beta2; A.eps = eps;
  A.bc1 = (float)(1.0 - pow((double)beta1, (double)step));         // Adam's bias corrections 1 - beta^t, rounded once
  A.bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  A.theta = theta; A.m = m; A.v = v; A.gate_out = gate_out; A.size_out = size_out; A.count_out = count_out;
  const int64_t items = (int64_t)n_rep * batch;
  hipLaunchKernelGGL(rgms::mask_step_kernel, dim3((unsigned)rg::ceil_div(items, rgms::MS_BLOCK / 64)), dim3(rgms::MS_BLOCK), 0,
                     (hipStream_t)stream, A);
  RG_LAUNCH_CHECK();
  return 0;
}
