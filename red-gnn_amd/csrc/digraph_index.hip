// The per-hop index of an edited r-digraph (rg_digraph_hop_ranges, rg_digraph_hop_index): what explain._hop_index builds in torch
// (nonzero over all E edges, searchsorted, unique_consecutive, int64 edge columns, validation read-backs) as a handful of launches
// that touch only the E_l edges of the hop.
//
// The digraph is explain's: edges int32 [E, 5] = (row, hop, head, rel, tail) ordered by (row, hop, tail), offsets int64 [B + 1].
//
//   rg_digraph_hop_ranges, once per rescore: one thread per (row b, hop l) finds, by binary search inside offsets[b]..offsets[b + 1],
//     the first edge of the row with hop >= l: hop_ptr[b][l - 1]; hop_ptr[b][L] = offsets[b + 1].  The host then forms, per hop, the
//     exclusive scan over the rows of the segment lengths (hop_first [L][B + 1]): the hop-l edges are the B segments
//     hop_ptr[b][l - 1] .. hop_ptr[b][l], and hop-l item i is edge hop_ptr[b][l - 1] + i - hop_first[l - 1][b] of the row b that a
//     binary search of i in hop_first[l - 1] gives.
//   rg_digraph_hop_index, per hop: flag_kernel (one thread per item: validate the edge, keep mask, binary search of (row, head) in the
//     previous hop's node keys), rg::scan_exclusive over the flags, compact_kernel (at / src / rel / edge_time / live, and the node key
//     (row, tail) of every live edge), start_kernel (a live edge starts a node iff its key differs from the one before it in the
//     compacted list), a second scan, node_kernel (keys, dst_ptr, row_of, prev_idx).  The counts and the status word come back in one
//     12-byte copy.
//
// Integer results only; every output position is a function of the scans, so no bit depends on the launch geometry.  Every index is
// clamped before it is used as an address: whatever the arrays hold, nothing outside them is touched, and what is wrong with them is
// reported through the status word (RG_DIGRAPH_INDEX_* in include/redgnn.h), with vector atomics.
#include <algorithm>
#include <vector>

#include "common.h"

namespace rgdi {
namespace {

constexpr int DI_BLOCK = 256;

__device__ __forceinline__ int64_t clamp64(int64_t x, int64_t lo, int64_t hi) { return x < lo ? lo : (x > hi ? hi : x); }

// (position, found) of `want` in the sorted, duplicate-free keys[0..n)
__device__ __forceinline__ bool find_key(const int64_t* __restrict__ keys, int32_t n, int64_t want, int32_t* pos) {
  int32_t lo = 0, hi = n;
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  *pos = lo;
  return lo < n && keys[lo] == want;
}

__global__ __launch_bounds__(DI_BLOCK) void ranges_kernel(const int32_t* __restrict__ edges, const int64_t* __restrict__ offsets,
                                                          int64_t E, int32_t B, int32_t L, int64_t* __restrict__ hop_ptr) {
  const int64_t tid = (int64_t)blockIdx.x * DI_BLOCK + threadIdx.x;
  if (tid >= (int64_t)B * L) return;
  const int32_t b = (int32_t)(tid / L), l = (int32_t)(tid - (int64_t)b * L) + 1;
  const int64_t beg = clamp64(offsets[b], 0, E), end = clamp64(offsets[b + 1], beg, E);
  int64_t lo = beg, hi = end;
  while (lo < hi) {                                      // the first edge of the row with hop >= l
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (edges[mid * 5 + 1] < l) lo = mid + 1; else hi = mid;
  }
  hop_ptr[(int64_t)b * (L + 1) + l - 1] = lo;
  if (l == L) hop_ptr[(int64_t)b * (L + 1) + L] = end;
}

struct DiArgs {
  const int32_t* edges;        // [E, 5]
  const uint8_t* keep;         // [E] or nullptr
  const int32_t* edge_time;    // [E] or nullptr
  const int64_t* hop_ptr;      // [B, L + 1]
  const int32_t* hop_first;    // [B + 1] of this hop
  const int64_t* keys_prev;    // [n_prev]
  int64_t E;
  int32_t B, L, l, n_hop, n_prev, n_ent, n_rela_rows;
  // scratch, n_hop elements each
  uint32_t* flag;              // the item is live; later: the live edge starts a node
  int32_t* pos;                // exclusive scan of flag
  int32_t* item_src;           // the head's position in keys_prev
  int32_t* item_edge;          // the item's edge index
  int64_t* live_key;           // (row, tail) of every live edge, compacted
  int32_t* counts;             // [0] n_live, [1] n_dst, [2] status
  // outputs
  int32_t* at; int32_t* src; int32_t* rel; int32_t* time_out;
  int64_t* keys; int32_t* dst_ptr; int32_t* row_of; int32_t* prev_idx;
  uint8_t* live;               // [E]
};

__global__ __launch_bounds__(DI_BLOCK) void flag_kernel(DiArgs A) {
  const int32_t i = blockIdx.x * DI_BLOCK + threadIdx.x;
  if (i >= A.n_hop) return;
  int32_t lo = 0, hi = A.B;                               // the row: the last b with hop_first[b] <= i
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (A.hop_first[mid + 1] <= i) lo = mid + 1; else hi = mid;
  }
  const int32_t b = min(lo, A.B - 1);
  const int32_t k = i - A.hop_first[b];
  const int64_t e = clamp64(A.hop_ptr[(int64_t)b * (A.L + 1) + A.l - 1] + k, 0, A.E - 1);
  const int32_t* ed = A.edges + e * 5;
  const int32_t row = ed[0], hop = ed[1], head = ed[2], r = ed[3], tail = ed[4];
  int32_t bad = 0;
  if (row != b || hop != A.l) bad |= RG_DIGRAPH_INDEX_ROW_HOP;
  if (head < 0 || head >= A.n_ent || tail < 0 || tail >= A.n_ent) bad |= RG_DIGRAPH_INDEX_ENTITY;
  if (r < 0 || r >= A.n_rela_rows) bad |= RG_DIGRAPH_INDEX_RELATION;
  if (k > 0 && e > 0 && tail < A.edges[(e - 1) * 5 + 4]) bad |= RG_DIGRAPH_INDEX_ORDER;   // the item before it is the same row's
  uint32_t f = 0;
  int32_t p = 0;
  if (!bad && (!A.keep || A.keep[e] != 0)) f = find_key(A.keys_prev, A.n_prev, (int64_t)b * A.n_ent + head, &p) ? 1u : 0u;
  A.flag[i] = f;
  A.item_src[i] = p;
  A.item_edge[i] = (int32_t)e;
  if (bad) atomicOr(A.counts + 2, bad);
}

__global__ __launch_bounds__(DI_BLOCK) void compact_kernel(DiArgs A) {
  const int32_t i = blockIdx.x * DI_BLOCK + threadIdx.x;
  if (i >= A.n_hop || !A.flag[i]) return;
  const int32_t j = min(max(A.pos[i], 0), A.n_hop - 1);
  const int64_t e = A.item_edge[i];                       // (clamped into 0..E-1 by flag_kernel)
  const int32_t* ed = A.edges + e * 5;
  A.at[j] = (int32_t)e;
  A.src[j] = A.item_src[i];
  A.rel[j] = ed[3];
  if (A.time_out) A.time_out[j] = A.edge_time[e];
  A.live_key[j] = (int64_t)ed[0] * A.n_ent + ed[4];       // (row and tail passed flag_kernel's range checks)
  A.live[e] = 1;
}

__global__ __launch_bounds__(DI_BLOCK) void start_kernel(DiArgs A) {
  const int32_t j = blockIdx.x * DI_BLOCK + threadIdx.x;
  if (j >= A.n_hop) return;
  const int32_t n_live = min(max(A.counts[0], 0), A.n_hop);
  A.flag[j] = j < n_live && (j == 0 || A.live_key[j] != A.live_key[j - 1]) ? 1u : 0u;
}

__global__ __launch_bounds__(DI_BLOCK) void node_kernel(DiArgs A) {
  const int32_t j = blockIdx.x * DI_BLOCK + threadIdx.x;
  if (j >= A.n_hop) return;
  const int32_t n_live = min(max(A.counts[0], 0), A.n_hop), n_dst = min(max(A.counts[1], 0), n_live);
  if (j == 0) A.dst_ptr[n_dst] = n_live;
  if (j >= n_live || !A.flag[j]) return;
  const int32_t n = min(max(A.pos[j], 0), A.n_hop - 1);
  const int64_t key = A.live_key[j];
  A.keys[n] = key;
  A.dst_ptr[n] = j;
  A.row_of[n] = (int32_t)(key / A.n_ent);
  int32_t p;
  A.prev_idx[n] = find_key(A.keys_prev, A.n_prev, key, &p) ? p : -1;
  if (A.l == A.L && j > 0 && A.live_key[j - 1] / A.n_ent == key / A.n_ent) atomicOr(A.counts + 2, RG_DIGRAPH_INDEX_TWO_TAILS);
}

size_t items_bytes(int64_t n_hop) { return rg::align_up((size_t)n_hop * 24, 256); }

}  // namespace
}  // namespace rgdi

extern "C" int rg_digraph_hop_ranges(const int32_t* edges, const int64_t* offsets, int64_t n_edges, int32_t batch, int32_t n_hops,
                                     int64_t* hop_ptr_out, int32_t* hop_first_out, int64_t* hop_ptr_host, int64_t* hop_edges_host,
                                     int32_t* status_host, void* stream) {
  const char* who = "rg_digraph_hop_ranges";
  RG_CHECK(n_edges >= 0 && n_edges < ((int64_t)1 << 31), "%s: n_edges=%lld (need 0 <= n_edges < 2^31)", who, (long long)n_edges);
  RG_CHECK(batch >= 0 && n_hops >= 1 && n_hops <= 32, "%s: batch=%d n_hops=%d (need batch >= 0, n_hops in 1..32)", who, batch, n_hops);
  RG_CHECK(hop_ptr_host && hop_edges_host && status_host, "%s: NULL argument (hop_ptr_host, hop_edges_host or status_host)", who);
  *status_host = 0;
  for (int32_t l = 0; l < n_hops; ++l) hop_edges_host[l] = 0;
  if (batch == 0) {
    RG_CHECK(n_edges == 0, "%s: %lld edges without a row", who, (long long)n_edges);
    return 0;
  }
  RG_CHECK(offsets && hop_ptr_out && hop_first_out && (edges || n_edges == 0), "%s: NULL argument", who);
  const int32_t B = batch, L = n_hops;
  hipStream_t s = (hipStream_t)stream;
  const int64_t threads = (int64_t)B * L;
  hipLaunchKernelGGL(rgdi::ranges_kernel, dim3((unsigned)rg::ceil_div(threads, rgdi::DI_BLOCK)), dim3(rgdi::DI_BLOCK), 0, s, edges, offsets,
                     n_edges, B, L, hop_ptr_out);
  RG_LAUNCH_CHECK();
  RG_HIP(hipMemcpyAsync(hop_ptr_host, hop_ptr_out, (size_t)B * (L + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  RG_HIP(hipStreamSynchronize(s));
  // per hop the exclusive scan of the rows' segment lengths; a row whose hops are not sorted gives ranges that the hop's own
  // validation refuses (an edge whose hop is not l), a row that starts below hop 1 is refused here
  std::vector<int32_t> first((size_t)L * (B + 1));
  for (int32_t l = 0; l < L; ++l) {
    int64_t run = 0;
    for (int32_t b = 0; b < B; ++b) {
      const int64_t* p = hop_ptr_host + (int64_t)b * (L + 1);
      first[(size_t)l * (B + 1) + b] = (int32_t)run;
      run += std::min(std::max(p[l + 1] - p[l], (int64_t)0), n_edges - run);      // (the total stays <= n_edges < 2^31)
      if (l == 0 && p[0] != (b == 0 ? 0 : p[-1])) *status_host |= RG_DIGRAPH_INDEX_ROW_HOP;   // (p[-1]: the row before ends there)
    }
    first[(size_t)l * (B + 1) + B] = (int32_t)run;
    hop_edges_host[l] = run;
  }
  // (a copy from pageable memory: the runtime is done with the vector when the call returns)
  RG_HIP(hipMemcpyAsync(hop_first_out, first.data(), first.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  RG_HIP(hipStreamSynchronize(s));
  return 0;
}

extern "C" size_t rg_digraph_hop_index_scratch_bytes(int64_t n_hop_edges) {
  if (n_hop_edges <= 0 || n_hop_edges >= ((int64_t)1 << 31)) return 0;
  return rgdi::items_bytes(n_hop_edges) + rg::align_up(rg::scan_scratch_elems(n_hop_edges) * 4, 256) + 256;
}

extern "C" int rg_digraph_hop_index(const int32_t* edges, const uint8_t* keep, const int32_t* edge_time, int64_t n_edges, int32_t batch,
                                    int32_t n_hops, int32_t hop, const int64_t* hop_ptr, const int32_t* hop_first, int64_t n_hop_edges,
                                    const int64_t* keys_prev, int64_t n_prev, int32_t n_ent, int32_t n_rela_rows, int32_t* at_out,
                                    int32_t* src_out, int32_t* rel_out, int32_t* time_out, int64_t* keys_out, int32_t* dst_ptr_out,
                                    int32_t* row_of_out, int32_t* prev_idx_out, uint8_t* live, void* scratch, size_t scratch_bytes,
                                    int64_t* n_live_host, int64_t* n_dst_host, int32_t* status_host, void* stream) {
  const char* who = "rg_digraph_hop_index";
  RG_CHECK(n_edges >= 0 && n_edges < ((int64_t)1 << 31), "%s: n_edges=%lld (need 0 <= n_edges < 2^31)", who, (long long)n_edges);
  RG_CHECK(batch >= 0 && n_hops >= 1 && n_hops <= 32 && hop >= 1 && hop <= n_hops, "%s: batch=%d n_hops=%d hop=%d (need batch >= 0, "
           "n_hops in 1..32, hop in 1..n_hops)", who, batch, n_hops, hop);
  RG_CHECK(n_hop_edges >= 0 && n_hop_edges <= n_edges, "%s: n_hop_edges=%lld (need 0 <= n_hop_edges <= n_edges = %lld)", who,
           (long long)n_hop_edges, (long long)n_edges);
  RG_CHECK(n_prev >= 0 && n_prev < ((int64_t)1 << 31), "%s: n_prev=%lld (need 0 <= n_prev < 2^31)", who, (long long)n_prev);
  RG_CHECK(n_ent >= 1 && n_rela_rows >= 1, "%s: n_ent=%d n_rela_rows=%d (need both positive)", who, n_ent, n_rela_rows);
  RG_CHECK(n_live_host && n_dst_host && status_host, "%s: NULL argument (n_live_host, n_dst_host or status_host)", who);
  *n_live_host = *n_dst_host = 0;
  *status_host = 0;
  if (n_hop_edges == 0 || n_prev == 0) return 0;          // no edge can be live: nothing is launched, the outputs are the caller's
  RG_CHECK(batch > 0, "%s: %lld edges of the hop without a row", who, (long long)n_hop_edges);
  RG_CHECK(edges && hop_ptr && hop_first && keys_prev && at_out && src_out && rel_out && keys_out && dst_ptr_out && row_of_out &&
           prev_idx_out && live, "%s: NULL argument", who);
  RG_CHECK((edge_time == nullptr) == (time_out == nullptr), "%s: edge_time and time_out go together (one of them is NULL)", who);
  const size_t need = rg_digraph_hop_index_scratch_bytes(n_hop_edges);
  RG_CHECK(scratch && scratch_bytes >= need && ((uintptr_t)scratch & 255) == 0, "%s: scratch %zu B < required %zu B (or not 256-B aligned)",
           who, scratch ? scratch_bytes : (size_t)0, need);
  RG_CHECK((((uintptr_t)keys_prev | (uintptr_t)keys_out | (uintptr_t)hop_ptr) & 7) == 0, "%s: int64 arrays must be 8-B aligned", who);

  rgdi::DiArgs A;
  A.edges = edges; A.keep = keep; A.edge_time = edge_time; A.hop_ptr = hop_ptr; A.hop_first = hop_first; A.keys_prev = keys_prev;
  A.E = n_edges; A.B = batch; A.L = n_hops; A.l = hop; A.n_hop = (int32_t)n_hop_edges; A.n_prev = (int32_t)n_prev; A.n_ent = n_ent;
  A.n_rela_rows = n_rela_rows;
  char* base = (char*)scratch;
  A.live_key = (int64_t*)base;                            // 8 B per item first: every slice stays aligned
  A.flag = (uint32_t*)(A.live_key + n_hop_edges);
  A.pos = (int32_t*)(A.flag + n_hop_edges);
  A.item_src = A.pos + n_hop_edges;
  A.item_edge = A.item_src + n_hop_edges;
  int32_t* scan_scr = (int32_t*)(base + rgdi::items_bytes(n_hop_edges));
  A.counts = (int32_t*)(base + need - 256);
  A.at = at_out; A.src = src_out; A.rel = rel_out; A.time_out = time_out; A.keys = keys_out; A.dst_ptr = dst_ptr_out; A.row_of = row_of_out;
  A.prev_idx = prev_idx_out; A.live = live;

  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)rg::ceil_div(n_hop_edges, rgdi::DI_BLOCK)), block(rgdi::DI_BLOCK);
  if (rg::zero_async(A.counts, 256, s)) return 1;
  hipLaunchKernelGGL(rgdi::flag_kernel, grid, block, 0, s, A);
  RG_LAUNCH_CHECK();
  if (rg::scan_exclusive(A.flag, A.pos, n_hop_edges, false, A.counts + 0, scan_scr, s)) return 1;
  hipLaunchKernelGGL(rgdi::compact_kernel, grid, block, 0, s, A);
  RG_LAUNCH_CHECK();
  hipLaunchKernelGGL(rgdi::start_kernel, grid, block, 0, s, A);
  RG_LAUNCH_CHECK();
  if (rg::scan_exclusive(A.flag, A.pos, n_hop_edges, false, A.counts + 1, scan_scr, s)) return 1;
  hipLaunchKernelGGL(rgdi::node_kernel, grid, block, 0, s, A);
  RG_LAUNCH_CHECK();
  int32_t got[3] = {0, 0, 0};
  RG_HIP(hipMemcpyAsync(got, A.counts, sizeof(got), hipMemcpyDeviceToHost, s));
  RG_HIP(hipStreamSynchronize(s));
  *n_live_host = std::min<int64_t>(std::max(got[0], 0), n_hop_edges);
  *n_dst_host = std::min<int64_t>(std::max(got[1], 0), *n_live_host);
  *status_host = got[2];
  return 0;
}
