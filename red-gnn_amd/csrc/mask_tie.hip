// Tied edge masks (rg_mask_tie_grad, rg_mask_tie_gates): the two launches that let explain.RDigraph.learn_mask learn one gate per
// GROUP of edges - a fact with all its copies, a (hop, relation) pair, any label - instead of one per edge.  Every member edge reads
// its group's gate, so the chain rule through the tie is a sum and the way back is a gather:
//
//   grp_grad[k, g] = sum over the members e of group g of grad[k, e]                      (rg_mask_tie_grad)
//   gate_out[k, e] = grp_gate[k, group_of[e]]  where group_of[e] >= 0                     (rg_mask_tie_gates)
//
// Between them runs rg_mask_step, unchanged, on the [n_rep, n_groups] arrays.
//
// The sum is DEFINED (include/redgnn.h states it; a float32 loop on the host reproduces it bit for bit): a group is cut into chunks of
// MASK_TIE_CHUNK members counted from its own first member, a chunk's sum starts from its first member's value and adds the rest in
// member order, and a group's sum is its chunk sums added in chunk order, starting from the first.  An empty group gives +0.
//
// Mapping (wave64, no LDS): a lane per (replica, item).  The first n_groups items are the groups themselves: a lane whose group has at
// most one chunk sums it and stores the result, a lane whose group is cut does nothing.  The other items are the chunks of the cut
// groups, listed by the host from grp_ptr_host (as rg_digraph_layer_fwd lists its cut destinations): such a lane stores its chunk's
// sum into a partial array, and a second launch adds a group's partial sums in chunk order - the project's split rule.  A lane loads
// eight member positions, then the eight values they name, and only then adds: the gathers are independent and in flight together,
// only the adds are ordered (a group of one member, most groups of a fact tie, is one load each).  Nothing is chosen from the call's
// sizes, so a (replica, group) sum has the same bits whatever else the call carries; no float atomics.
//
// rg_mask_tie_gates is memory-bound: a lane takes four consecutive edges, one 16-byte load of their groups and - where all four are
// tied - one 16-byte store of their gates (dword-aligned: replica k's array starts at k * n_edges); a group of four with an edge that
// is not tied, or the array's last partial four, stores per element, and nothing is stored where an edge is not tied.
#include <vector>

#include "common.h"

namespace rgmt {
namespace {

constexpr int TIE_CHUNK = RG_MASK_TIE_CHUNK;      // members per chunk of a group (include/redgnn.h)
constexpr int TIE_FLIGHT = 8;                     // gathers a lane keeps in flight
constexpr int TIE_BLOCK = 256;
static_assert(TIE_CHUNK % TIE_FLIGHT == 0, "a chunk is whole passes of the gather");

struct __attribute__((aligned(4))) f4u { float x, y, z, w; };        // a 16-byte access that is only dword-aligned
struct __attribute__((aligned(4))) i4u { int32_t x, y, z, w; };

// members lo .. hi of one replica's grad (at most TIE_CHUNK of them, at least one), added in member order from the first one's value
__device__ __forceinline__ float chunk_sum(const int32_t* __restrict__ member, const float* __restrict__ grad, int n_edges, int lo, int hi) {
  if (hi - lo == 1) return grad[min(max(member[lo], 0), n_edges - 1)];      // (most groups of a fact tie: one load each, the value's bits)
  float acc = 0.f;
  for (int p = lo; p < hi; p += TIE_FLIGHT) {
    float x[TIE_FLIGHT];
#pragma unroll
    for (int u = 0; u < TIE_FLIGHT; ++u) {
      const int q = min(p + u, hi - 1);                  // (past the end: the last member once more, never added)
      x[u] = grad[min(max(member[q], 0), n_edges - 1)];
    }
#pragma unroll
    for (int u = 0; u < TIE_FLIGHT; ++u)
      if (p + u < hi) acc = (p + u == lo) ? x[u] : acc + x[u];
  }
  return acc;
}

struct TgArgs {
  int n_rep, n_groups, n_items, n_chunks, n_edges, n_member;
  const int32_t* grp_ptr;
  const int32_t* member;
  const int4* chunks;          // {group, first member, end, slot} of every chunk of a cut group
  const float* grad;
  float* grp_grad;
  float* partial;              // [n_rep, n_chunks]
};

__global__ __launch_bounds__(TIE_BLOCK) void mask_tie_grad_kernel(TgArgs A) {
  const int64_t tid = (int64_t)blockIdx.x * TIE_BLOCK + threadIdx.x;
  if (tid >= (int64_t)A.n_rep * A.n_items) return;
  const int k = (int)(tid / A.n_items), item = (int)(tid - (int64_t)k * A.n_items);
  const float* grad = A.grad + (int64_t)k * A.n_edges;
  if (item < A.n_groups) {
    const int lo = min(max(A.grp_ptr[item], 0), A.n_member);
    const int hi = min(max(A.grp_ptr[item + 1], lo), A.n_member);
    if (hi - lo > TIE_CHUNK) return;                     // a cut group: its chunks are items of their own
    A.grp_grad[(int64_t)k * A.n_groups + item] = hi > lo ? chunk_sum(A.member, grad, A.n_edges, lo, hi) : 0.f;
  } else {
    const int4 c = A.chunks[item - A.n_groups];          // (the host's list: checked against n_member there)
    A.partial[(int64_t)k * A.n_chunks + c.w] = chunk_sum(A.member, grad, A.n_edges, c.y, c.z);
  }
}

// the cut groups: their chunks' partial sums added in chunk order, the first one initialising the sum
__global__ __launch_bounds__(TIE_BLOCK) void mask_tie_combine_kernel(const int4* __restrict__ hubs, int n_hubs, int n_rep, int n_chunks,
                                                                     int n_groups, const float* __restrict__ partial,
                                                                     float* __restrict__ grp_grad) {
  const int64_t tid = (int64_t)blockIdx.x * TIE_BLOCK + threadIdx.x;
  if (tid >= (int64_t)n_rep * n_hubs) return;
  const int k = (int)(tid / n_hubs);
  const int4 hub = hubs[tid - (int64_t)k * n_hubs];      // {group, first slot, chunks, -}
  const float* p = partial + (int64_t)k * n_chunks + hub.y;
  float acc = p[0];
  for (int c = 1; c < hub.z; ++c) acc += p[c];
  grp_grad[(int64_t)k * n_groups + hub.x] = acc;
}

__global__ __launch_bounds__(TIE_BLOCK) void mask_tie_gates_kernel(int n_rep, int n_edges, int n_groups, int n_quads,
                                                                   const int32_t* __restrict__ group_of,
                                                                   const float* __restrict__ grp_gate, float* __restrict__ gate_out) {
  const int64_t tid = (int64_t)blockIdx.x * TIE_BLOCK + threadIdx.x;
  if (tid >= (int64_t)n_rep * n_quads) return;
  const int k = (int)(tid / n_quads);
  const int e0 = (int)(tid - (int64_t)k * n_quads) * 4;
  const float* gg = grp_gate + (int64_t)k * n_groups;
  float* out = gate_out + (int64_t)k * n_edges;
  if (e0 + 4 <= n_edges) {
    const i4u g = *(const i4u*)(group_of + e0);
    if ((g.x | g.y | g.z | g.w) >= 0) {                  // all four tied (no sign bit among them)
      const int top = n_groups - 1;
      *(f4u*)(out + e0) = f4u{gg[min(g.x, top)], gg[min(g.y, top)], gg[min(g.z, top)], gg[min(g.w, top)]};
      return;
    }
  }
  const int n = min(n_edges - e0, 4);
  for (int i = 0; i < n; ++i) {
    const int g = group_of[e0 + i];
    if (g >= 0) out[e0 + i] = gg[min(g, n_groups - 1)];
  }
}

// the cut groups of a group pointer on the host: how many, how many chunks they make, and the chunks of all groups together
// (first_bad, if asked for: the first group whose pointer decreases, or -1)
void count_cuts(const int32_t* ptr, int32_t n_groups, int64_t* n_hubs, int64_t* n_chunks, int64_t* all_chunks, int32_t* first_bad = nullptr) {
  *n_hubs = *n_chunks = *all_chunks = 0;
  for (int32_t g = 0; g < n_groups; ++g) {
    const int64_t len = (int64_t)ptr[g + 1] - ptr[g];
    if (len < 0 && first_bad && *first_bad < 0) *first_bad = g;
    if (len <= 0) continue;
    const int64_t c = rg::ceil_div(len, TIE_CHUNK);
    *all_chunks += c;
    if (c > 1) { ++*n_hubs; *n_chunks += c; }
  }
}

size_t list_bytes(int64_t n_hubs, int64_t n_chunks) { return rg::align_up((size_t)(n_hubs + n_chunks) * sizeof(int4), 256); }

size_t scratch_need(int64_t n_hubs, int64_t n_chunks, int64_t n_rep) {
  return n_hubs ? list_bytes(n_hubs, n_chunks) + rg::align_up((size_t)(n_rep * n_chunks) * sizeof(float), 256) : 0;
}

}  // namespace
}  // namespace rgmt

extern "C" size_t rg_mask_tie_grad_scratch_bytes(const int32_t* grp_ptr_host, int32_t n_groups, int32_t n_rep) {
  if (!grp_ptr_host || n_groups <= 0 || n_rep < 1) return 0;   // (rg_mask_tie_grad reports what is wrong with them)
  int64_t n_hubs, n_chunks, all_chunks;
  rgmt::count_cuts(grp_ptr_host, n_groups, &n_hubs, &n_chunks, &all_chunks);
  return rgmt::scratch_need(n_hubs, n_chunks, n_rep);
}

extern "C" int rg_mask_tie_grad(int32_t n_rep, int64_t n_edges, int32_t n_groups, int64_t n_member, const int32_t* grp_ptr,
                                const int32_t* grp_ptr_host, const int32_t* member, const float* grad, float* grp_grad, void* scratch,
                                size_t scratch_bytes, void* stream) {
  const char* who = "rg_mask_tie_grad";
  RG_CHECK(n_rep >= 1, "%s: n_rep=%d (need at least one replica)", who, n_rep);
  RG_CHECK(n_edges >= 0 && n_groups >= 0 && n_member >= 0, "%s: n_edges=%lld n_groups=%d n_member=%lld (negative size)", who,
           (long long)n_edges, n_groups, (long long)n_member);
  RG_CHECK((int64_t)n_rep * n_edges < ((int64_t)1 << 31) && (int64_t)n_rep * n_groups < ((int64_t)1 << 31) &&
           n_member < ((int64_t)1 << 31),
           "%s: n_rep=%d times n_edges=%lld or n_groups=%d, or n_member=%lld, overflows int32", who, n_rep, (long long)n_edges, n_groups,
           (long long)n_member);
  RG_CHECK(grp_ptr && grp_ptr_host && member && grad && grp_grad, "%s: NULL argument", who);
  RG_CHECK(grp_ptr_host[0] == 0, "%s: grp_ptr starts at %d, not 0", who, grp_ptr_host[0]);
  int32_t first_bad = -1;
  int64_t n_hubs, n_chunks, all_chunks;                  // (one pass over the host array: a group that decreases counts as empty)
  rgmt::count_cuts(grp_ptr_host, n_groups, &n_hubs, &n_chunks, &all_chunks, &first_bad);
  RG_CHECK(first_bad < 0, "%s: grp_ptr decreases at group %d", who, first_bad);
  RG_CHECK(grp_ptr_host[n_groups] == n_member, "%s: grp_ptr ends at %d, not at the number of members %lld", who, grp_ptr_host[n_groups],
           (long long)n_member);
  RG_CHECK(n_member == 0 || n_edges > 0, "%s: %lld members but no edge to name", who, (long long)n_member);
  RG_CHECK((int64_t)n_rep * all_chunks < ((int64_t)1 << 31) && (int64_t)n_rep * ((int64_t)n_groups + n_chunks) < ((int64_t)1 << 31),
           "%s: n_rep=%d times %lld chunks overflows int32", who, n_rep, (long long)all_chunks);
  const size_t need = rgmt::scratch_need(n_hubs, n_chunks, n_rep);
  RG_CHECK(need == 0 || (scratch && scratch_bytes >= need), "%s: scratch %zu B < required %zu B", who, scratch ? scratch_bytes : (size_t)0,
           need);
  RG_CHECK(need == 0 || ((uintptr_t)scratch & 15) == 0, "%s: scratch must be 16-B aligned", who);
  if (n_groups == 0) return 0;                           // nothing to sum and nothing launched
  hipStream_t s = (hipStream_t)stream;
  int4* hubs_dev = (int4*)scratch;
  rgmt::TgArgs A;
  A.n_rep = n_rep; A.n_groups = n_groups; A.n_items = (int)(n_groups + n_chunks); A.n_chunks = (int)n_chunks; A.n_edges = (int)n_edges;
  A.n_member = (int)n_member; A.grp_ptr = grp_ptr; A.member = member; A.chunks = n_hubs ? hubs_dev + n_hubs : nullptr; A.grad = grad;
  A.grp_grad = grp_grad;
  A.partial = n_hubs ? (float*)((char*)scratch + rgmt::list_bytes(n_hubs, n_chunks)) : nullptr;
  if (n_hubs) {
    std::vector<int4> list((size_t)(n_hubs + n_chunks));
    int64_t h = 0, slot = 0;
    for (int32_t g = 0; g < n_groups; ++g) {
      const int32_t lo = grp_ptr_host[g], hi = grp_ptr_host[g + 1];
      if (hi - lo <= rgmt::TIE_CHUNK) continue;
      const int n_c = (int)rg::ceil_div(hi - lo, rgmt::TIE_CHUNK);
      list[h++] = make_int4(g, (int)slot, n_c, 0);
      for (int c = 0; c < n_c; ++c, ++slot)
        list[n_hubs + slot] = make_int4(g, lo + c * rgmt::TIE_CHUNK, (int)std::min((int64_t)hi, (int64_t)lo + (int64_t)(c + 1) * rgmt::TIE_CHUNK),
                                        (int)slot);
    }
    // (a copy from pageable memory: the runtime is done with the vector when the call returns)
    RG_HIP(hipMemcpyAsync(hubs_dev, list.data(), list.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  }
  const int64_t threads = (int64_t)n_rep * A.n_items;
  hipLaunchKernelGGL(rgmt::mask_tie_grad_kernel, dim3((unsigned)rg::ceil_div(threads, rgmt::TIE_BLOCK)), dim3(rgmt::TIE_BLOCK), 0, s, A);
  RG_LAUNCH_CHECK();
  if (n_hubs) {
    hipLaunchKernelGGL(rgmt::mask_tie_combine_kernel, dim3((unsigned)rg::ceil_div((int64_t)n_rep * n_hubs, rgmt::TIE_BLOCK)),
                       dim3(rgmt::TIE_BLOCK), 0, s, (const int4*)hubs_dev, (int)n_hubs, n_rep, (int)n_chunks, n_groups,
                       (const float*)A.partial, grp_grad);
    RG_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int rg_mask_tie_gates(int32_t n_rep, int64_t n_edges, int32_t n_groups, const int32_t* group_of, const float* grp_gate,
                                 float* gate_out, void* stream) {
  const char* who = "rg_mask_tie_gates";
  RG_CHECK(n_rep >= 1, "%s: n_rep=%d (need at least one replica)", who, n_rep);
  RG_CHECK(n_edges >= 0 && n_groups >= 0, "%s: n_edges=%lld n_groups=%d (negative size)", who, (long long)n_edges, n_groups);
  RG_CHECK((int64_t)n_rep * n_edges < ((int64_t)1 << 31) && (int64_t)n_rep * n_groups < ((int64_t)1 << 31),
           "%s: n_rep=%d times n_edges=%lld or n_groups=%d overflows int32", who, n_rep, (long long)n_edges, n_groups);
  RG_CHECK(group_of && grp_gate && gate_out, "%s: NULL argument", who);
  if (n_edges == 0 || n_groups == 0) return 0;           // no gate to hand on and nothing launched: the caller owns gate_out
  const int n_quads = (int)rg::ceil_div(n_edges, 4);
  const int64_t threads = (int64_t)n_rep * n_quads;
  hipLaunchKernelGGL(rgmt::mask_tie_gates_kernel, dim3((unsigned)rg::ceil_div(threads, rgmt::TIE_BLOCK)), dim3(rgmt::TIE_BLOCK), 0,
                     (hipStream_t)stream, n_rep, (int)n_edges, n_groups, n_quads, group_of, grp_gate, gate_out);
  RG_LAUNCH_CHECK();
  return 0;
}
