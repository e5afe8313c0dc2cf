/*
 * redgnn.h — C-ABI of the MI355X-native RED-GNN hot path (libredgnn.so).
 *
 * The reference (LARS-research/RED-GNN) is pure Python and has no FFI; its boundary is the
 * nn.Module API of RED_GNN_trans plus the DataLoader.get_neighbors callback
 * (Static/transductive/models.py:45-89, load_data.py:106-131).  This header is the native
 * boundary *behind* that API: every entry point names the reference code it replaces.
 * All paths below are relative to Static/transductive/ of the reference.
 *
 * Conventions
 *   - plain C types only: device pointers (const float* / const int32_t*), sizes, an opaque
 *     stream (hipStream_t passed as void*).  No torch types.
 *   - every function returns 0 on success, non-zero on error; rg_last_error() then returns a
 *     thread-local message.  Nothing is printed, nothing aborts.
 *   - buffers are caller-owned.  The library allocates device memory only inside rg_graph
 *     handles; per-batch state lives in a caller-provided workspace (rg_frontier).
 *   - launches go to the stream passed in and are asynchronous, except rg_frontier_expand,
 *     which returns the new node/edge counts and therefore synchronises that stream once.
 *   - indices are int32 (requires B*n_ent < 2^31 and n_fact < 2^31; checked).
 *   - node order is the reference's: sorted by (batch_idx, entity); node id = rank in that order.
 */
#ifndef REDGNN_H
#define REDGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rg_graph rg_graph;        /* device-resident KG: CSR by head and CSR by tail */
typedef struct rg_frontier rg_frontier;  /* per-batch visited-set state inside a caller workspace */

const char* rg_last_error(void);
int rg_version(void);
/* number of memset nodes in a captured hipGraph_t (-1 on error).  The library issues its fills as kernels because replayed graphs
 * with several memset nodes misbehaved on ROCm 7.2; the host side asserts that nothing else put one into a captured forward. */
int rg_hipgraph_fill_nodes(void* hip_graph);

/* ---- graph build: replaces load_data.py:69-81 (double_triple + load_graph) ------------------
 * triples: HOST int32 [n,3] = (head, rel, tail) base triples.  If add_inverse != 0 the inverse
 * (tail, rel+n_rel, head) of every triple is added (load_data.py:69-74).  One identity row
 * (e, 2*n_rel, e) per entity is always added (load_data.py:77-79).  Fact-row order is kept
 * inside every CSR row so sums are reproducible. */
int rg_graph_create(int32_t n_ent, int32_t n_rel, const int32_t* triples_host, int64_t n,
                    int add_inverse, rg_graph** out);
/* The same graph from a DEVICE triple array (int32 [n,3]), built on the device: the per-epoch rebuild of shuffle_train
 * (load_data.py:152-164: permute facts + train, re-split 3:1, load_graph) without moving the triples or the CSR arrays through the host.
 * Every array of the result equals rg_graph_create's on the same triples.  Synchronises `stream` (it returns counts). */
int rg_graph_create_device(int32_t n_ent, int32_t n_rel, const int32_t* triples_dev, int64_t n,
                           int add_inverse, void* stream, rg_graph** out);
/* copy the word-parallel walk's packs back (tests): sizes first (out arrays NULL), then ent int32 [n_packs*128, 2], pack int32 [n_packs, 4],
 * rows int32 [n_vrows, 2]; and the virtual rows of the CSR-by-tail, int32 [n_vrows, 4]. */
int rg_graph_export_packs(const rg_graph* g, int32_t* n_packs, int32_t* n_vrows, int32_t* ent_host, int32_t* pack_host, int32_t* rows_host,
                          int32_t* vrows_host);
/* temporal graph (T-RED-GNN interpolation): replaces the per-call coo_matrix build of
 * Temporal/interpolation/model_cuda.py:121-126 over the quadruple array of graph.py:34-49.
 * quads: HOST int32 [n,4] = (head, rel, tail, time id), used as given (the reference's graph array already
 * holds the identity rows with the sentinel timestamp); n_rela_rows = rows of the relation tables. */
int rg_tgraph_create(int32_t n_ent, int32_t n_rela_rows, int32_t n_time, const int32_t* quads_host, int64_t n,
                     rg_graph** out);
/* The same graph without the rows listed in exclude_rows_host (row indices into quads, duplicates allowed): the training
 * mode of T_RED_GNN.forward, `dataset = np.delete(self.dataset, batch['example_idx'], axis=0)` (model_cuda.py:103-104),
 * without a host copy of the array per batch. */
int rg_tgraph_create_excluding(int32_t n_ent, int32_t n_rela_rows, int32_t n_time, const int32_t* quads_host, int64_t n,
                               const int64_t* exclude_rows_host, int64_t n_exclude, rg_graph** out);
int rg_graph_destroy(rg_graph* g);
int64_t rg_graph_n_fact(const rg_graph* g);      /* rows incl. inverse + identity (load_data.py:80) */
/* copy the device CSR back (tests): ptr arrays have n_ent+1 entries, pair arrays 2*n_fact. */
int rg_graph_export(const rg_graph* g, int32_t* out_ptr_host, int32_t* out_rel_tail_host,
                    int32_t* in_ptr_host, int32_t* in_head_rel_host);
/* copy the out-list ordered by tail back (tests; static graphs only): a second CSR-by-head over the same out_ptr in which every head's
 * out-edges are ordered by (tail, position of the edge in the CSR-by-tail), so that the edges head -> t appear in the order the
 * CSR-by-tail lists them - the order every walk of rg_layer_fwd sums a destination in.  rel_tail_host int32 [n_fact, 2] = {rel, tail},
 * pos_host int32 [n_fact] = the edge's index in in_head_rel, packed_host uint32 [n_fact] = (rel << 20 | tail) (an error where the graph
 * has no packed entries: n_ent > 2^20 or more than 2^12 relation rows).  Any pointer may be NULL. */
int rg_graph_export_out_by_tail(const rg_graph* g, int32_t* rel_tail_host, int32_t* pos_host, uint32_t* packed_host);
/* copy the time ids of a temporal graph's CSR entries back (tests): out_time_host int32 [n_fact] beside out_rel_tail, in_time_host
 * int32 [n_fact] beside in_head_rel (either may be NULL).  With them a test can name the CSR position of an edge whose (head, rel,
 * tail) repeats at several times.  An error on static graphs. */
int rg_graph_export_time(const rg_graph* g, int32_t* out_time_host, int32_t* in_time_host);
/* copy any other array of the graph back by name (tests), and its scalars.  Arrays, all of 32-bit words, as [rows, cols]:
 *   rel_ptr [n_rela_rows+1], rel_ht [n_fact, 2] = {head, tail}, rel_tm [n_fact]       the CSR by relation (rel_tm: temporal graphs)
 *   time_ptr [n_time+1], time_ht [n_fact, 2] = {head, tail}, time_rel [n_fact]         the CSR by time id (temporal graphs)
 *   in_pk, out_pk, out_bt_pk uint32 [n_fact]          the packed entries beside in_head_rel, out_rel_tail and the out-list by tail
 *   in_vr_rows, out_vr_rows, rel_vr_rows, time_vr_rows [n, 4] = {row id, first entry, length, slot or -1}: the virtual rows of the CSR by
 *       tail, by head, by relation and by time id, sorted by length descending; *_vr_split [n_split, 4] = {row id, first slot, segments, 0}
 * Sizes first: dims_out int64 [2] = {rows, cols} (may be NULL); an array this graph does not have (packed entries of a wide graph, the
 * time arrays of a static one) gives rows = -1 and is no error, a name not in the list is one.  out_host (may be NULL) receives rows *
 * cols words.  scalars_out int64 [15] (may be NULL) = n_fact, max_in_deg, max_out_deg, then n, n_split, n_slots of in_vr, out_vr, rel_vr
 * and time_vr.  name may be NULL (scalars only). */
int rg_graph_export_array(const rg_graph* g, const char* name, int64_t* dims_out, void* out_host, int64_t* scalars_out);

/* ---- frontier expansion: replaces DataLoader.get_neighbors, load_data.py:106-131 ------------
 * A frontier keeps `n_levels` visited-set snapshots: level 0 = the query nodes, level k = after
 * k hops.  Levels are stored modulo n_levels: 2 is enough for inference (ping-pong), training
 * keeps n_layer+1 so that rg_layer_bwd can revisit every hop. */
size_t rg_frontier_workspace_bytes(int32_t n_ent, int32_t batch, int32_t n_levels);
/* workspace: device memory of at least rg_frontier_workspace_bytes(), 256-B aligned. */
int rg_frontier_create(int32_t n_ent, int32_t batch, int32_t n_levels, void* workspace_dev,
                       size_t workspace_bytes, rg_frontier** out);
int rg_frontier_destroy(rg_frontier* f);
/* level 0 frontier {(b, q_sub[b])}: models.py:73.  q_sub: device int32 [batch]. */
int rg_frontier_reset(rg_frontier* f, const int32_t* q_sub_dev, void* stream);
/* level 0 frontier from an arbitrary node set (the general form get_neighbors accepts,
 * load_data.py:106,115): nodes device int32 [n,2] = (batch, entity), batch < `batch`, no duplicates. */
int rg_frontier_reset_nodes(rg_frontier* f, const int32_t* nodes_dev, int64_t n, void* stream);
/* one hop: new frontier = tails of all out-edges of the current one (identity edges keep the
 * old nodes).  counts_host[0] = N_new, counts_host[1] = E (edges of this hop),
 * counts_host[2] = N_old, counts_host[3] = new level.  Synchronises `stream`. */
int rg_frontier_expand(rg_frontier* f, const rg_graph* g, int64_t* counts_host, void* stream);
/* The same hop without the read-back: nothing synchronises, so a whole forward (models.py:69-88) can be enqueued - or
 * captured into a hipGraph - in one go.  The level's N stays on the device (rg_frontier_count_ptr; consumed by
 * rg_dense_fwd_dev), and while a level's size is unknown on the host rg_layer_fwd / rg_tlayer_fwd take their n_new as
 * an estimate (> 0, it only picks the walk) and need agg_out sized for batch * n_ent rows.
 * rg_frontier_level_counts reads N and E of levels 0..current back: counts_host[2*l] = N_l, [2*l+1] = E_l
 * (room for 2 * 16 values; synchronises `stream`). */
int rg_frontier_expand_async(rg_frontier* f, const rg_graph* g, void* stream);
/* rg_frontier_expand_async + rg_frontier_nodes (nodes_out [batch*n_ent, 2], prev_idx_out [batch*n_ent]; either may be NULL) in one
 * call: for small batches (batch * ceil(n_ent/32) <= 12288 words) the level build and the node list are ONE single-workgroup launch
 * instead of six, which is what a replayed graph at the reference's n_tbatch = 50 is made of (launch latency, not work). */
int rg_frontier_expand_nodes_async(rg_frontier* f, const rg_graph* g, int32_t* nodes_out, int32_t* prev_idx_out, void* stream);
/* After an asynchronous expansion the hop's edge count is not known on the host; a caller that knows what to expect (from an eager run of
 * the same shape) says so: it only tunes the work distribution of the next rg_layer_fwd (any value is correct).  Cleared by the next expansion. */
int rg_frontier_set_edge_hint(rg_frontier* f, int64_t n_edges);
const int32_t* rg_frontier_count_ptr(const rg_frontier* f);
int rg_frontier_level_counts(const rg_frontier* f, int64_t* counts_host, void* stream);
/* nodes of the current level: nodes_out int32 [N_new,2] = (batch, entity) sorted
 * (== tail_nodes, load_data.py:123); prev_idx_out int32 [N_new] = index of the node in the
 * previous level or -1; old_nodes_new_idx_out int32 [N_old] (load_data.py:127-129).
 * Any pointer may be NULL. */
int rg_frontier_nodes(const rg_frontier* f, int32_t* nodes_out, int32_t* prev_idx_out,
                      int32_t* old_nodes_new_idx_out, void* stream);
/* materialised edge list of hop `level-1 -> level` (API parity with sampled_edges,
 * load_data.py:118-125): edges_out int32 [E,6] = (batch, head, rel, tail, old_idx, new_idx),
 * grouped by new_idx (destination-segmented) and, inside a destination, in the order the
 * CSR-by-tail lists its in-edges (fact-row order); row_ptr_out int32 [N_new+1].
 * nodes_new: device int32 [N_new,2] from rg_frontier_nodes (may be NULL where N_new == 0:
 * row_ptr_out = {0}).  scratch: device memory of rg_frontier_edges_scratch_bytes(N_new) bytes.
 * `level` must still be resident together with its source level: level in
 * (current - n_levels + 1, current].  An error on a frontier that has windows set
 * (rg_frontier_set_window): the edge list of a windowed hop is not materialised. */
size_t rg_frontier_edges_scratch_bytes(int64_t n_new);
int rg_frontier_edges(const rg_frontier* f, const rg_graph* g, int32_t level,
                      const int32_t* nodes_new, int64_t n_new, int32_t* edges_out,
                      int32_t* row_ptr_out, void* scratch_dev, void* stream);

/* ---- layer forward: replaces GNNLayer.forward models.py:29-39 incl. torch_scatter.scatter ----
 * For hop level-1 -> level:
 * agg[o] = sum over in-edges e=(s,r,o) of alpha_e * (hidden[s] + rela[r]),
 * alpha_e = sigmoid(w_alpha . relu(a_s[s] + a_r[r] + a_q[b]) + b_alpha), with the hoisted
 * projections a_s = hidden Ws^T [N_old,ap], a_r = rela Wr^T [2R+1,ap], a_q = rela[q_rel] Wqr^T + b [B,ap]
 * (ap = attention dim padded to a multiple of 4, pad columns zero).  Edges are enumerated
 * from the CSR-by-tail of `g` and the frontier bitmaps; no edge list is materialised.
 * hidden [N_old, ld], rela [2R+1, ld], agg_out [N_new, ld] (every row is written);
 * ld % 4 == 0, ld >= d, pad columns of hidden/rela must be zero.  n_new is checked against the
 * frontier.  scratch: device memory of rg_layer_fwd_scratch_bytes() bytes (partial sums of hub
 * destinations that are cut into segments), 16-B aligned.
 *
 * walk (0 .. 8): how the edges are enumerated (the sums and their order are the same; results are bitwise equal):
 *   0  let the library pick from the sizes of the hop (known on the host after rg_frontier_expand);
 *   1  per-query walk: every live destination tests its KG in-edges against the previous frontier;
 *   2 .. 7  word-parallel walk for hops whose SOURCE frontier is sparse (as the reference expands from the frontier's
 *      nodes, load_data.py:115-118): 32 / 16 / 8 / 4 / 2 / 1 queries per work item straight from the entity-major bitmaps; only for
 *      level == the newest hop of a static graph.
 *   8  single-source walk, hop 0 of a query batch: level == 1 of a frontier started by rg_frontier_reset (one node per query, its
 *      subject, which the frontier keeps) on a static graph.  Every query enumerates its subject's out-edges from an out-list ordered by
 *      tail, in runs of equal tail, and forms each destination's whole sum in one place (no partial rows, no second launch); hidden
 *      and a_s are read at row b of query b.  Any other level or frontier: an error.  What walk 0 runs whenever it applies.
 * rg_layer_fwd_plan returns what walk 0 would pick among the general walks 1 .. 7 for given sizes (n_old, n_new nodes, n_edges of the
 * hop), and rg_layer_fwd_single_source whether walk 8 applies to `level` (1 or 0), which walk 0 then takes ahead of that plan: callers
 * that enqueue without read-backs (rg_frontier_expand_async) record the code from an eager run and pass it explicitly.
 * rg_layer_fwd_wp_tickets returns the work items a wave takes per queue ticket (1 .. 32) that rg_layer_fwd would give the word-parallel
 * walk `walk` (2 .. 7) on `level` if called now - sized from the hop's edge count as the frontier holds it (known after
 * rg_frontier_expand, else the value of rg_frontier_set_edge_hint, else unknown) - and the walk's number of work items in *n_items_out
 * (may be NULL); 0 (and 0 items) for a walk that takes no such tickets (0, 1, 8) or a graph without packed entries.  It steers
 * speed only; tests read it to know which ticket sizes they ran. */
size_t rg_layer_fwd_scratch_bytes(const rg_frontier* f, const rg_graph* g, int32_t ld);
int rg_layer_fwd_plan(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, int64_t n_new,
                      int64_t n_edges, int32_t ld);
int rg_layer_fwd_wp_tickets(const rg_frontier* f, const rg_graph* g, int32_t level, int32_t walk, int64_t* n_items_out);
int rg_layer_fwd_single_source(const rg_frontier* f, const rg_graph* g, int32_t level);
int rg_layer_fwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_new,
                 const float* hidden, const float* rela, int32_t d, int32_t ld,
                 const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                 const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                 float* agg_out, void* scratch_dev, size_t scratch_bytes, int32_t walk, void* stream);

/* ---- hoisted attention tables of ALL layers in one launch: models.py:33,36 (Wr_attn, Wqr_attn applied per relation / per query
 * instead of per edge).  For layer l: a_r_out[l][r][ap] = rela[l][r] . Wr[l][j], a_q_out[l][b][ap] = rela[l][q_rel[b]] . Wqr[l][j] + bqr[l][j]
 * (columns j >= attn_dim zero), rela_pad_out[l][r][ld] = rela[l][r] zero-padded to ld columns (NULL when ld == d).
 * rela / Wr / Wqr / bqr: HOST arrays of n_layer device pointers (tables [n_rela_rows, d], weights [attn_dim, d], bias [attn_dim]);
 * q_rel device int64 [batch].  n_layer <= 16. */
int rg_attn_tables(int32_t n_layer, int32_t n_rela_rows, int32_t batch, int32_t d, int32_t ld, int32_t attn_dim, int32_t ap,
                   const float* const* rela, const float* const* Wr, const float* const* Wqr, const float* const* bqr,
                   const int64_t* q_rel, float* a_r_out, float* a_q_out, float* rela_pad_out, void* stream);

/* ---- temporal layer forward: replaces Temporal/interpolation/model_cuda.py:149-160,192 ------------------
 * agg[o] = sum_e alpha_e * (hidden_dir[3 s + dir_e] + rela_dir[dir_e * n_rela_rows + r] + time_dir[dir_e * n_time + |dt_e|]),
 * dt_e = time(e) - q_time[b], dir = 0 (dt<0, past) / 1 (dt=0, now) / 2 (dt>0, future): the three direction
 * linears applied per node / relation / |dt| by the caller (W(h+r+tau) = Wh + Wr + Wtau);
 * alpha_e as in rg_layer_fwd with a_s, a_r, a_q the three blocks of attention_1 (no biases: pass b_alpha = 0).
 * q_time device int32 [B]; hidden_dir [3*N_old, ld]; rela_dir [3*n_rela_rows, ld]; time_dir [3*n_time, ld].
 * Scratch as rg_layer_fwd_scratch_bytes(). */
int rg_tlayer_fwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_new, const int32_t* q_time,
                  const float* hidden_dir, const float* rela_dir, const float* time_dir, int32_t d, int32_t ld,
                  const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                  const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                  float* agg_out, void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- temporal EXTRAPOLATION (Temporal/extrapolation/model_cuda_new_embedding.py:135-265): every query sees only the data rows of
 * its own time window, `self.dataset[time_offset_list[begin]:time_offset_list[cur_t]]` (:167-171), plus one self-loop per entity.
 * The graph is an rg_tgraph whose quadruples carry, in the time field, the index of the edge's row in the time-sorted data array
 * (self-loops: any value >= n_data).  rg_frontier_set_window gives the frontier the per-query row windows [win_lo[b], win_hi[b])
 * (device int32 [batch], caller-owned, NULL = no windows): rg_frontier_expand* then follow only edges valid for the query, and
 * rg_xlayer_fwd is the layer (:186-226) over those edges.  All edges lie in the past, so one direction matrix applies (past_linear):
 * hidden_p = W_past h [N_old, ld], rela_p = W_past rela [n_rela_rows, ld], time_p [n_tab, ld] = W_past time_embed(delta) for
 * delta = 0..n_tab-1; delta(edge, b) = q_time[b] - row_time[data row] (self-loops: q_time[b] - loop_time[b]), clamped to n_tab - 1.
 * Attention as rg_tlayer_fwd.  Its adjoint is rg_xlayer_bwd (below, with rg_tlayer_bwd). */
int rg_frontier_set_window(rg_frontier* f, const int32_t* win_lo_dev, const int32_t* win_hi_dev, int32_t n_data);
int rg_xlayer_fwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_new, const int32_t* q_time,
                  const int32_t* loop_time, const int32_t* row_time, int32_t n_data,
                  const float* hidden_p, const float* rela_p, const float* time_p, int32_t n_tab, int32_t d, int32_t ld,
                  const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                  const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                  float* agg_out, void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- layer backward: adjoint of rg_layer_fwd (autograd of models.py:29-39) --------------------
 * grad_agg [N_new, ld].  grad_hidden [N_old, ld] and grad_a_s [N_old, ap] are WRITTEN (every row);
 * grad_rela [2R+1, ld], grad_a_r [2R+1, ap], grad_w_alpha [attn_dim], grad_b_alpha [1] are ACCUMULATED
 * into (caller zero-fills).  grad_a_q [B, ap] (may be NULL) is WRITTEN: the per-query segment sum of grad_a_s
 * (a_s[s] and a_q[b] enter the attention as a sum).  n_old is checked against the frontier.
 * scratch: rg_layer_bwd_scratch_bytes() bytes. */
size_t rg_layer_bwd_scratch_bytes(const rg_frontier* f, const rg_graph* g, int32_t ld, int32_t ap);
int rg_layer_bwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old,
                 const float* hidden, const float* rela, int32_t d, int32_t ld,
                 const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                 const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                 const float* grad_agg,
                 float* grad_hidden, float* grad_rela, float* grad_a_s, float* grad_a_r, float* grad_a_q,
                 float* grad_w_alpha, float* grad_b_alpha,
                 void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- temporal layer backward: adjoint of rg_tlayer_fwd (autograd of Temporal/interpolation/model_cuda.py:149-160,192) ----
 * Arguments as rg_tlayer_fwd.  grad_hidden_dir [N_old, 3*ld] (row s = the three direction rows 3s..3s+2) and
 * grad_a_s [N_old, ap] are WRITTEN (every row); grad_rela_dir [3*n_rela_rows, ld], grad_time_dir [3*n_time, ld],
 * grad_a_r [n_rela_rows, ap], grad_w_alpha [attn_dim] are ACCUMULATED into (caller zero-fills); grad_a_q [B, ap] (may
 * be NULL) is WRITTEN, the per-query segment sum of grad_a_s.  The direction linears are differentiated by the caller
 * (three GEMMs on these sums).  Needs a graph from rg_tgraph_create. */
size_t rg_tlayer_bwd_scratch_bytes(const rg_frontier* f, const rg_graph* g, int32_t ld, int32_t ap);
int rg_tlayer_bwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, const int32_t* q_time,
                  const float* hidden_dir, const float* rela_dir, const float* time_dir, int32_t d, int32_t ld,
                  const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                  const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                  const float* grad_agg,
                  float* grad_hidden_dir, float* grad_rela_dir, float* grad_time_dir, float* grad_a_s, float* grad_a_r,
                  float* grad_a_q, float* grad_w_alpha,
                  void* scratch_dev, size_t scratch_bytes, void* stream);

/* Adjoint of rg_xlayer_fwd (training of the extrapolation setting, Temporal/extrapolation/main.py:296-320 around
 * model_cuda_new_embedding.py:186-239).  Arguments as rg_xlayer_fwd (the frontier still carries the batch's windows: rg_frontier_set_window).
 * grad_hidden_p [N_old, ld] and grad_a_s [N_old, ap] are WRITTEN; grad_rela_p [n_rela_rows, ld], grad_time_p [n_tab, ld],
 * grad_a_r [n_rela_rows, ap], grad_w_alpha [attn_dim] are ACCUMULATED into (caller zero-fills); grad_a_q [B, ap] (may be NULL) is
 * WRITTEN.  past_linear and the periodic time embedding are differentiated by the caller.  scratch: rg_tlayer_bwd_scratch_bytes(). */
int rg_xlayer_bwd(const rg_frontier* f, const rg_graph* g, int32_t level, int64_t n_old, const int32_t* q_time,
                  const int32_t* loop_time, const int32_t* row_time, int32_t n_data,
                  const float* hidden_p, const float* rela_p, const float* time_p, int32_t n_tab, int32_t d, int32_t ld,
                  const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                  const float* w_alpha, const float* b_alpha, int32_t attn_dim,
                  const float* grad_agg,
                  float* grad_hidden_p, float* grad_rela_p, float* grad_time_p, float* grad_a_s, float* grad_a_r,
                  float* grad_a_q, float* grad_w_alpha,
                  void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- dense epilogue of a layer (inference): replaces models.py:41 (W_h + act), :81 (h0 index_copy_, as a
 * gather by prev_idx), :82-84 (single-step nn.GRU; dropout = identity in eval), the next layer's
 * Ws_attn projection (:36, hoisted per node) and, on the last layer, :86-88 (W_final + scatter into
 * scores_all).  One f32-MFMA kernel; weights in the layouts of the reference's state dict:
 * W_h [d,d], weight_ih_l0 / weight_hh_l0 [3d,d] (gate rows r,z,n), bias_* [3d], Ws_next [attn,d] or NULL,
 * W_final [d] or NULL.  agg [n,ld], hidden_prev [n_old,ld], prev_idx int32 [n] (-1 = new node; NULL = all
 * new), a_s_out [n,ap], nodes int32 [n,2], scores_all [B*n_ent] (pre-zeroed; only visited entries are
 * written), hidden_out [n,ld] - or NULL on the last layer (W_final given, Ws_next NULL), when nobody reads the new state: the kernels then
 * skip its stores and the scores are bit for bit the same; NULL in any other call is an error.  Rows are written whole up to the
 * kernels' padded width (32 columns for d <= 32, 64 for d <= 64, 128; columns of a wider ld are left alone): with zero pad columns
 * d .. ld - 1 in agg and hidden_prev, the pad columns of hidden_out are exactly 0 (the padded weights and biases are zero, so a pad
 * element is 0.5 tanh(0) + 0.5 h0_pad), and a_s_out columns attn_dim .. ap - 1 are exactly 0.  The new state does not depend on
 * which of Ws_next / W_final a call carries, nor on n_hint of rg_dense_fwd_dev (bit for bit, at every precision).
 * act: 0 identity, 1 relu, 2 tanh.  Supported: d <= 64 or d == 128, attn_dim <= 16
 * (rg_dense_fwd_supported); other shapes return an error and the caller keeps its own dense path. */
int rg_dense_fwd_supported(int32_t d, int32_t attn_dim);
int rg_dense_fwd(int64_t n, int32_t d, int32_t ld, const float* agg, const float* hidden_prev,
                 const int32_t* prev_idx, const float* W_h, int32_t act,
                 const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                 const float* Ws_next, int32_t attn_dim, int32_t ap, float* a_s_out,
                 const float* W_final, const int32_t* nodes, int32_t n_ent, float* scores_all,
                 float* hidden_out, int32_t precision, void* scratch, int64_t scratch_bytes, void* stream);
/* scratch: device memory of rg_dense_scratch_bytes(d, precision) bytes, 256-B aligned (0 bytes / NULL for every case but d = 128 with
 * precision 1 or 2, whose weights stream through LDS from a split image written there first).  Contents are dead after the call. */
int64_t rg_dense_scratch_bytes(int32_t d, int32_t precision);
/* precision: how the matrix products are evaluated.
 *   0  v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation (what the reference's fp32 GEMMs compute up to sum order)
 *   1  every fp32 operand as a two-term f16 split (22 significant bits, per-row power-of-two scaling), three
 *      v_mfma_f32_16x16x32_f16 per product with fp32 accumulation: errors of a few 1e-7 of a dot product's largest terms instead
 *      of 1e-7, at 3/16 of the matrix-pipe time
 *   2  every fp32 operand as an EXACT three-term f16 split (hi + mid + lo = all 24 bits; csrc/split3.h), the six partial products of
 *      order >= 2^-22 per product on v_mfma_f32_16x16x32_f16 / _bf8_bf8 with fp32 accumulation: fp32 arithmetic (operands exact,
 *      products good to 2^-31, fp32 sums) at 6/16 of the matrix-pipe time of precision 0.  The model's default. */

/* Test hook of precision 2's operand form: splits each of the n_rows rows of `cols` floats on the device exactly as the dense kernels
 * do (row scale = the power of two that takes the row's largest magnitude to [2^14, 2^15)) and writes back[n_rows, cols] =
 * (hi + mid + lo) / scale - bitwise equal to x for every element within 2^-15 of its row's largest magnitude (smaller ones: within 2^-39 of that largest) - and, if parts is not
 * NULL, parts[n_rows, cols, 4] = {hi, mid, lo, the bf8 (weights') form of lo}, scaled. */
int rg_split3_roundtrip(const float* x, int64_t n_rows, int32_t cols, float* back, float* parts, void* stream);
/* Test hook of precision 2's products: runs the d <= 64 kernel of rg_dense_fwd(precision = 2) on rows of d floats (ld = d) and writes
 * out[n, d] = one of its matrix products instead of the new state: which = 1: act(W_h agg); 2: weight_ih[2d:3d] x with
 * x = act(W_h agg); 3: weight_hh[2d:3d] h0 (h0 = hidden_prev gathered by prev_idx).  With one-hot operand rows (times powers of two)
 * a product is a column of the weight matrix and must come out bit for bit: the six partial products of csrc/split3.h are all there. */
int rg_split3_product_check(int32_t which, int64_t n, int32_t d, const float* agg, const float* hidden_prev, const int32_t* prev_idx,
                            const float* W_h, int32_t act, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                            float* out, void* stream);

/* ---- weight gradients of the dense training step: out[m, n] = G^T X (row-major) for G [n_rows, m] (row stride ldg), X [n_rows, n] (row
 * stride ldx), n_rows in the millions, m <= 192, n <= 64 (wider products: call per column block) - autograd of models.py:41 (W_h),
 * :83 (weight_ih / weight_hh of the GRU) and the hoisted :36 Ws_attn.  colsum [m] (may be NULL) = column sums of G (the bias
 * gradients).  Exact fp32 products on v_mfma_f32_16x16x4_f32, rows read once, per-wave partial results added in a fixed order
 * (bitwise reproducible).  scratch: rg_gram_tn_scratch_bytes(m, n) bytes. */
size_t rg_gram_tn_scratch_bytes(int32_t m, int32_t n);
int rg_gram_tn(const float* g, int64_t ldg, int32_t m, const float* x, int64_t ldx, int32_t n, int64_t n_rows, float* out, float* colsum,
               void* scratch_dev, size_t scratch_bytes, void* stream);

/* ---- filtered ranking: replaces utils.py:7-14 cal_ranks (+ the filter loop base_model.py:107-115)
 * scores device fp32 [B, n_ent]; answers / filters as CSR over queries (device int32):
 * ans_ptr [B+1], ans_idx [ans_ptr[B]], filt_ptr [B+1], filt_idx [..].  ranks_out device fp32
 * [ans_ptr[B]] in (query, answer-list) order: rank = #{j not in filter: s'_j > s'_a} +
 * (#{j: s'_j == s'_a} + 1)/2 with s' = fl32(fl32(s - rowmin) + 1e-8). */
int rg_rank(const float* scores, int32_t batch, int32_t n_ent,
            const int32_t* ans_ptr, const int32_t* ans_idx,
            const int32_t* filt_ptr, const int32_t* filt_idx,
            float* ranks_out, void* stream);

/* ---- filtered top-k prediction: the k best new answers of each query row (models.py RED_GNN_trans.predict)
 * scores device fp32 [batch, n_ent] (contiguous, the readout's output).  q_key int64 [batch]: key = s * (2*n_rel + 1) + r of the row.
 * Known-answer index (device): known_keys int64 [n_keys] sorted ascending and unique, known_ptr int64 [n_keys + 1], known_idx int32:
 * the tails of key i are known_idx[known_ptr[i]:known_ptr[i+1]], ascending and unique.  n_keys = 0 (arrays may be NULL): exclude
 * nothing.  Each row drops the tails its key lists (binary search of known_keys on the device) and returns in idx_out int32
 * [batch, k] / score_out fp32 [batch, k] the remaining entities ordered by score descending, then entity id ascending; -0.0 ranks
 * equal to +0.0, NaN below -inf (returned only when nothing else is left).  Fewer than k remaining: the row's tail is idx -1,
 * score -inf.  score_out holds scores[row, idx] bit for bit.  1 <= k <= 1024, n_ent any positive int32.  Each row depends only on
 * its own inputs; results are deterministic (integer atomics only).  Known tails outside 0..n_ent-1 are ignored; a known list that
 * is not ascending and unique breaks the contract: the row's result is then unspecified (it may differ from the top-k and from run
 * to run), though nothing is read or written out of bounds. */
int rg_topk(const float* scores, int32_t batch, int32_t n_ent, int32_t k, const int64_t* q_key,
            const int64_t* known_keys, const int64_t* known_ptr, const int32_t* known_idx, int64_t n_keys,
            int32_t* idx_out, float* score_out, void* stream);

/* ---- ranks of the extrapolation setting: replaces segment_rank_fil (Temporal/extrapolation/segment.py:346-387)
 * scores device fp32 [n_pairs] and ent device int32 [n_pairs]: score and entity of every visited (query, entity) pair; query q owns
 * the pairs seg_ptr[q]:seg_ptr[q+1] (device int32 [batch+1], or int64 when seg_ptr_is64 != 0; an empty segment is legal, bounds
 * outside 0..n_pairs are clamped).  Entities are unique within a segment, in any order.  target device int32 [batch].
 * Two known-object indexes in rg_topk's layout (keys int64 sorted and unique, ptr int64 [n_keys + 1], idx int32 ascending and
 * unique per key; n_keys = 0 with NULL arrays: filter nothing): sp_* by (s, p), spt_* by (s, p, t), with the queries' keys key_sp /
 * key_spt device int64 [batch].  A key its index lacks filters nothing (the reference's defaultdict).
 * With ts the score of the target's pair, each output is #{kept j: s_j > ts} + (#{kept j: s_j == ts} - 1)/2 + 1 (IEEE comparisons:
 * a NaN score counts for nothing): rank_out keeps every pair of the segment, rank_fil_out / rank_fil_t_out those whose entity is
 * not in the key's list of sp_* / spt_*, the target itself always kept.  found_out int32 [batch] = 1; a target that is not in its
 * segment gets found = 0 and 1e9 in all three ranks.  Integer counting only: each query depends on its own inputs alone and the
 * results are bitwise reproducible.  No limit on segment or list length. */
int rg_segment_rank(const float* scores, const int32_t* ent, int64_t n_pairs, const void* seg_ptr, int32_t seg_ptr_is64,
                    const int32_t* target, int32_t batch,
                    const int64_t* key_sp, const int64_t* sp_keys, const int64_t* sp_ptr, const int32_t* sp_idx, int64_t n_sp,
                    const int64_t* key_spt, const int64_t* spt_keys, const int64_t* spt_ptr, const int32_t* spt_idx, int64_t n_spt,
                    float* rank_out, float* rank_fil_out, float* rank_fil_t_out, int32_t* found_out, void* stream);

/* ---- filtered top-k of the extrapolation setting: the forecasts of (s, p, ?, t) among the entities the query's window reaches
 * (T_RED_GNN.predict of extrapolation.py) - what rg_topk is for a dense row, in rg_segment_rank's layout.
 * scores (the logits) / ent / n_pairs / seg_ptr / seg_ptr_is64 / batch as rg_segment_rank: entities unique within a segment, in any
 * order; bounds clamped to 0..n_pairs; an empty segment is legal; a segment holds fewer than 2^31 pairs.  One known-object index
 * in rg_topk's layout (known_keys / known_ptr / known_idx / n_keys) with the queries' keys q_key int64 [batch]: n_keys = 0 with NULL
 * arrays excludes nothing, a key the index lacks excludes nothing, known entities that are not in the segment are ignored.
 * idx_out int32 [batch, k] / score_out fp32 [batch, k], 1 <= k <= 1024: per query the pairs whose entity is not in the key's list,
 * ordered by score descending, then entity id ascending, with rg_topk's key order (NaN lowest, -0 == +0); score_out is the input
 * score bit for bit; past the end -1 / -inf.  prob_out fp32 [batch, k] (may be NULL; past the end 0): the per-query softmax over ALL
 * pairs of the segment, excluded ones included (scatter_softmax of model_cuda_new_embedding.py:248), exp(s - m) / sum_j exp(s_j - m)
 * with m the segment's maximum, both reduced in a fixed order (per-thread strided partials, wave shuffle, waves in index order): a
 * query's probabilities are bitwise reproducible and do not depend on the rest of the batch.  A NaN score (or m = +-inf) makes the
 * segment's probabilities NaN.  One workgroup per query; integer atomics only in the selection; each query depends on its own
 * segment and list alone.  A known list of up to 256 entities is searched in LDS, a longer one in memory; a segment of up to 24576
 * pairs keeps its keys and kept flags in LDS, a longer one is re-read on every pass of the select.  Nothing outside [0, n_pairs) or
 * outside the index arrays is read; a known list that is not ascending gives an unspecified, in-bounds result, as for rg_topk. */
int rg_segment_topk(const float* scores, const int32_t* ent, int64_t n_pairs, const void* seg_ptr, int32_t seg_ptr_is64,
                    int32_t batch, int32_t k, const int64_t* q_key, const int64_t* known_keys, const int64_t* known_ptr,
                    const int32_t* known_idx, int64_t n_keys, int32_t* idx_out, float* score_out, float* prob_out, void* stream);

/* ---- evaluation of the interpolation setting: the per-query loss term and filtered rank counts of the validation loop of
 * Temporal/interpolation/main.py:125-183 (F.softmax over [B, n_ent], nll_loss(log(p + 1e-12)), topk, argsort, .item() per query),
 * in rg_segment_rank's layout, without the [B, n_ent] matrix.
 * scores (the logits) / ent / n_pairs / seg_ptr / seg_ptr_is64 / target / batch as rg_segment_rank: entities unique within a segment
 * and inside 0..n_ent-1, in any order; bounds clamped to 0..n_pairs; an empty segment is legal.  n_ent > 0: the width of the dense
 * row.  Two known-answer indexes in rg_topk's layout, a_* and b_*, with the queries' keys key_a / key_b int64 [batch]: n_keys = 0
 * with NULL arrays filters nothing, a key the index lacks filters nothing, listed entities outside 0..n_ent-1 are ignored.
 * Everything is defined on the dense row x[e] = the score of the pair (query, e) if the segment has one, else +0.0 - which is never
 * built.  With t the target, ts = x[t], n_seg the segment's length and n_zero = n_ent - n_seg:
 *   logp_out fp32 [batch] = log(exp(ts - m) / Z + 1e-12), m = max_e x[e] (0 takes part only if n_zero > 0), Z = sum_seg exp(s_j - m)
 *     + n_zero exp(-m), the second term only formed when n_zero > 0 (on a full row of very negative scores exp(-m) overflows): the
 *     per-row term of main.py:146.  expf / logf; m and the sum reduced in a fixed order (per-thread strided
 *     partials, wave shuffle, waves in index order).  A NaN score anywhere in the segment makes logp NaN.
 *   count_out int32 [batch, 6] = (gt, eq) for three keep-sets - every entity; the entities not in the key's list of a_*; of b_* - the
 *     target always kept: gt = #{kept e: x[e] > ts}, eq = #{kept e != t: x[e] == ts} (IEEE comparisons: NaN counts for nothing,
 *     -0.0 == +0.0).  The implicit zeros are counted arithmetically: a list L hides #{x in L, 0 <= x < n_ent, x != t} - #{pairs whose
 *     entity is in L, != t} of them, n_zero - [t not visited] - hidden are kept and join gt if 0 > ts, eq if 0 == ts.
 *   visited_out int32 [batch] = 1 if the target has a pair in the segment.  A target without one is no error: it scores 0 and ranks
 *     among the zeros, as the reference's dense argsort ranks it.
 * One workgroup of 256 threads per query; integer counters; each query depends on its own segment and lists alone and its results
 * are bitwise reproducible.  A known list of up to 256 entities is searched in LDS, a longer one in memory.  No limit on segment or
 * list length.  Nothing outside [0, n_pairs) or outside the index arrays is read; a list that is not ascending and unique gives an
 * unspecified, in-bounds result, as for rg_topk. */
int rg_segment_eval(const float* scores, const int32_t* ent, int64_t n_pairs, const void* seg_ptr, int32_t seg_ptr_is64,
                    const int32_t* target, int32_t batch, int32_t n_ent,
                    const int64_t* key_a, const int64_t* a_keys, const int64_t* a_ptr, const int32_t* a_idx, int64_t n_a,
                    const int64_t* key_b, const int64_t* b_keys, const int64_t* b_ptr, const int32_t* b_idx, int64_t n_b,
                    float* logp_out, int32_t* count_out, int32_t* visited_out, void* stream);

/* ---- the k best paths behind an answer: a selection on the compact r-digraph of rg_explain_* (explain.RDigraph), no counterpart
 * in the reference (model_cuda_rule_vis.py enumerates with networkx.all_simple_paths).
 * edges int32 [E, 5] = (row, hop, head, rel, tail) ordered by (row, hop, tail, CSR position), alpha fp32 [E], offsets int64 [B + 1]
 * non-decreasing with offsets[B] <= E (the caller checks that; everything read from the edge list itself is bounded by the row's
 * offsets, so a malformed list gives wrong paths, never an access outside the arrays).  n_hops = L in 1..32, k in 1..8.
 * A path of row b is L of its edges e_1..e_L with hop(e_l) = l, tail(e_l) = head(e_l+1) and e_L in the run of (hop, tail) that ends
 * the row, which must be a hop-L run; every hop-1 edge starts one.  Its product is ((1.0 * a_1) * a_2) ... * a_L in float64.  P comes
 * before Q at level l if P's product is larger; else if P's last edge has the smaller (head, rel, edge index); else, with the same
 * last edge, if P's prefix comes before Q's at level l - 1.  Per row the first min(k, number of paths) paths in that order:
 *   path_edge int64 [B, k, L] edge indices (-1 past the count), path_prod float64 [B, k] (0 past it), path_count int32 [B].
 * Rows row_lo..row_hi-1 are computed (rows of the full arrays: the outputs are indexed by the row itself), one workgroup per row,
 * and scratch holds rg_paths_scratch_bytes(offsets[row_hi] - offsets[row_lo], k) bytes (0: n_edges or k out of range).  A row's
 * result depends on its own edges alone, bit for bit, however the rows are cut into calls. */
size_t rg_paths_scratch_bytes(int64_t n_edges, int32_t k);
int rg_paths_topk(const int32_t* edges, const float* alpha, const int64_t* offsets, int32_t row_lo, int32_t row_hi, int32_t n_hops,
                  int32_t k, void* scratch, int64_t* path_edge, double* path_prod, int32_t* path_count, void* stream);

/* ---- one message-passing layer over an explicit edge list: rg_layer_fwd's arithmetic on the edges the caller hands over instead of
 * the ones a frontier and a graph enumerate (explain.RDigraph.rescore: an answer re-scored on its r-digraph with edges masked out).
 * The hop has n_dst destinations; dst_ptr int32 [n_dst + 1] is a CSR over its n_edges edges (device memory; dst_ptr_host is the same
 * array in host memory, read before anything is enqueued: it must start at 0, never decrease and end at n_edges).  Per edge src_idx
 * (its row in hidden [n_src, ld] and a_s [n_src, ap]) and rel (its row in rela [n_rela_rows, ld] and a_r [n_rela_rows, ap]); per
 * destination row_of_dst (its row in a_q [batch, ap]); w_alpha [attn_dim], b_alpha [1].  Indices outside their table are clamped to
 * it, never followed.
 *   alpha_e = sigmoid(w . relu((a_s[s] + a_r[r]) + a_q[b]) + b_alpha)      the forward family's order: on bit-identical inputs the very
 *                                                                         float rg_layer_fwd multiplies by and rg_explain_emit stores
 *   agg_out[o] = sum over the edges of o, in list order, of alpha_e * (hidden[s] + rela[r])        [n_dst, ld], every row written whole
 *   alpha_out [n_edges] = alpha_e, or NULL
 * Pad columns d .. ld - 1 of agg_out are 0 when those of hidden and rela are.  ld % 4 == 0, d <= ld <= 256; ap one of the padded
 * attention widths 4, 8, 12, 16, 32.  No float atomics: a destination of more than RG_DIGRAPH_CHUNK edges is cut into chunks of that
 * many, counted from its own first edge, which separate waves sum into partial rows in scratch; a second launch adds them in chunk
 * order.  agg_out[o] therefore has the same bits on every run and whatever else the call carries.  scratch: device memory of
 * rg_digraph_layer_fwd_scratch_bytes(dst_ptr_host, n_dst, ld) bytes, 16-B aligned (0 / NULL when no destination is cut, or the CSR is
 * malformed).  n_dst == 0 or n_edges == 0 succeeds and launches nothing (agg_out is then left alone).  The call waits for the copy of
 * the chunk list when a destination is cut; it is not for stream capture. */
#define RG_DIGRAPH_CHUNK 128
size_t rg_digraph_layer_fwd_scratch_bytes(const int32_t* dst_ptr_host, int32_t n_dst, int32_t ld);
int rg_digraph_layer_fwd(int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr, const int32_t* dst_ptr_host, const int32_t* src_idx,
                         const int32_t* rel, const int32_t* row_of_dst, int32_t n_src, int32_t n_rela_rows, int32_t batch,
                         const float* hidden, const float* rela, int32_t d, int32_t ld, const float* a_s, const float* a_r,
                         const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha, int32_t attn_dim, float* agg_out,
                         float* alpha_out, void* scratch, size_t scratch_bytes, void* stream);

/* ---- ... with a time per edge: rg_tlayer_fwd's arithmetic (n_dir = 3, temporal interpolation) or rg_xlayer_fwd's (n_dir = 1, the
 * extrapolation form) on an explicit edge list (explain.RDigraph.rescore of a temporal r-digraph).  Everything rg_digraph_layer_fwd
 * states holds - the same kernel with the time path compiled in, the same split rule, scratch size and argument checks - plus:
 * edge_time int32 [n_edges], q_time int32 [batch], time_tab [n_dir * n_time, ld] (16-B aligned), n_time > 0, n_dir 1 or 3.  hidden
 * then has n_dir * n_src rows and rela n_dir * n_rela_rows; a_s keeps n_src rows and a_r n_rela_rows: the attention reads the
 * un-directed s and r, so alpha_e is the float of rg_digraph_layer_fwd (pass b_alpha = 0: the temporal attention has no bias).
 *   n_dir == 3:  dt = edge_time[e] - q_time[b], dir = 0 (dt < 0) / 1 (dt == 0) / 2 (dt > 0)
 *                m_e = hidden[3 s + dir] + (rela[dir * n_rela_rows + r] + time_tab[dir * n_time + min(|dt|, n_time - 1)])
 *   n_dir == 1:  edge_time[e] is the day the caller resolved for the edge (a data row's day; a self-loop's: the first day of the
 *                query's window), m_e = hidden[s] + (rela[r] + time_tab[clamp(q_time[b] - edge_time[e], 0, n_time - 1)])
 *   agg_out[o] = sum over the edges of o, in list order, of alpha_e * m_e (fmaf)
 * The time row is clamped into its table whatever the times hold. */
int rg_digraph_tlayer_fwd(int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr, const int32_t* dst_ptr_host, const int32_t* src_idx,
                          const int32_t* rel, const int32_t* edge_time, const int32_t* row_of_dst, const int32_t* q_time, int32_t n_src,
                          int32_t n_rela_rows, int32_t batch, int32_t n_time, int32_t n_dir, const float* hidden, const float* rela,
                          const float* time_tab, int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                          const float* w_alpha, const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out, void* scratch,
                          size_t scratch_bytes, void* stream);

/* ---- the adjoint of one rg_digraph_layer_fwd hop (static form; the timed forms follow) with respect to a gate on every edge, the source states and
 * their attention projection (csrc/digraph_bwd.hip; explain.RDigraph.saliency).  With a gate g_e on the message of edge e,
 * agg[o] = sum_e g_e alpha_e (hidden[s] + rela[r]), the call returns the gradients at g == 1 of a scalar whose gradient with respect
 * to agg is grad_agg [n_dst, ld].  rela, a_r, a_q, w_alpha and b_alpha are CONSTANTS here: there are no parameter gradients, and the
 * gate does not enter alpha_e.  Per edge e = (s, r, o), b = row_of_dst[o], G = grad_agg:
 *   alpha_e = sigmoid(w . relu((a_s[s] + a_r[r]) + a_q[b]) + b_alpha)      attn_acc_fwd / attn_alpha: the float the forward multiplied by
 *   g_alpha = <G[o], hidden[s] + rela[r]>
 *   grad_gate[e]    = alpha_e * g_alpha                                    [n_edges], by position in the destination-ordered list
 *   grad_hidden[s] += alpha_e * G[o]                                       [n_src, ld], every row written whole (no edges: zeros)
 *   grad_a_s[s]    += g_alpha * alpha_e * (1 - alpha_e) * w * 1[pre > 0]   [n_src, ap], every row written whole
 * grad_hidden and grad_a_s may both be NULL (hop 1 of an r-digraph: its state is the constant 0); grad_gate then has the bits it has
 * with them.  Pad columns of the outputs are 0 when those of the inputs are.
 * The edges are the forward's destination-ordered list (rel [n_edges], row_of_dst [n_dst]) seen by source: src_ptr int32 [n_src + 1]
 * is a CSR over positions k (device; src_ptr_host the same array in host memory, read before anything is enqueued: it must start at
 * 0, never decrease and end at n_edges), edge_of [n_edges] the position in the destination-ordered list of the edge at k - a stable
 * permutation, so a source's edges keep their list order - and dst_of_edge [n_edges] the destination of the edge at list position e.
 * Indices outside their table are clamped to it, never followed.  ld % 4 == 0, d <= ld <= 256; ap one of 4, 8, 12, 16, 32.
 * No float atomics: a source of more than RG_DIGRAPH_CHUNK out-edges is cut into chunks of that many, counted from its own first
 * edge, which separate waves sum into partial rows in scratch; a second launch adds them in chunk order.  Every output therefore has
 * the same bits on every run and whatever else the call carries.  scratch: device memory of
 * rg_digraph_layer_bwd_scratch_bytes(src_ptr_host, n_src, ld, ap) bytes, 16-B aligned (0 / NULL when no source is cut, or the CSR is
 * malformed).  n_src == 0 or n_edges == 0 succeeds and launches nothing (the outputs are then left alone).  The call waits for the
 * copy of the chunk list when a source is cut; it is not for stream capture. */
size_t rg_digraph_layer_bwd_scratch_bytes(const int32_t* src_ptr_host, int32_t n_src, int32_t ld, int32_t ap);
int rg_digraph_layer_bwd(int32_t n_src, int32_t n_dst, int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host,
                         const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel, const int32_t* row_of_dst,
                         int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld,
                         const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                         int32_t attn_dim, const float* grad_agg, float* grad_gate, float* grad_hidden, float* grad_a_s, void* scratch,
                         size_t scratch_bytes, void* stream);

/* ---- ... of one rg_digraph_tlayer_fwd hop: the timed forms (n_dir = 3, temporal interpolation; n_dir = 1, the extrapolation form).
 * Everything rg_digraph_layer_bwd states holds - the same kernel with the time path compiled in, the same split rule and argument
 * checks, plus the forward's (n_dir 1 or 3, n_time > 0, three rows per source and relation within int32) - with these differences.
 * The message is m_e = hidden[hrow] + (rela[rrow] + time_tab[trow]), the rows formed exactly as rg_digraph_tlayer_fwd forms them
 * from edge_time int32 [n_edges] (by position in the destination-ordered list) and q_time int32 [batch]: 64-bit differences, |dt|
 * clamped to n_time - 1, the n_dir = 1 lag clamped to 0 .. n_time - 1; alpha_e reads the un-directed s and r (pass b_alpha = 0).
 *   g_alpha = <G[o], m_e>
 *   grad_gate[e]        = alpha_e * g_alpha
 *   grad_hidden[hrow]  += alpha_e * G[o]                                       [n_dir * n_src, ld]
 *   grad_a_s_dir[hrow] += g_alpha * alpha_e * (1 - alpha_e) * w * 1[pre > 0]   [n_dir * n_src, ap]: the caller adds a source's n_dir rows
 * The work item is a DIRECTED source row u = n_dir * s + dir (dir = 0 for n_dir = 1), and the source view is segmented by it:
 * src_ptr [n_dir * n_src + 1] (and src_ptr_host), edge_of the stable sort of the edges by u.  hidden has n_dir * n_src rows, rela
 * n_dir * n_rela_rows, time_tab n_dir * n_time, a_s n_src and a_r n_rela_rows.  The kernel forms an edge's direction again from its
 * times for rrow and trow, every index clamped into its table.  A directed row without edges is written as zeros; chunks are counted
 * per directed row.  scratch: rg_digraph_layer_bwd_scratch_bytes(src_ptr_host, n_dir * n_src, ld, ap) - the function only reads the
 * CSR it is handed, so it serves both forms with the number of rows of that CSR. */
int rg_digraph_tlayer_bwd(int32_t n_src, int32_t n_dst, int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host,
                          const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel, const int32_t* edge_time,
                          const int32_t* row_of_dst, const int32_t* q_time, int32_t n_rela_rows, int32_t batch, int32_t n_time,
                          int32_t n_dir, const float* hidden, const float* rela, const float* time_tab, int32_t d, int32_t ld,
                          const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                          int32_t attn_dim, const float* grad_agg, float* grad_gate, float* grad_hidden, float* grad_a_s_dir,
                          void* scratch, size_t scratch_bytes, void* stream);

/* ---- rg_digraph_layer_fwd with a gate on every edge's message, for n_rep >= 1 replicas of the hop in one launch (static form only;
 * explain.RDigraph.integrated_gradients, and rescore / saliency with gate=).  Everything rg_digraph_layer_fwd states holds - the same
 * kernel with the gate compiled in, the same split rule per replica and the same argument checks - plus: t float [n_rep] (device),
 * gate_lo float [n_edges] or NULL (meaning 0) and gate_hi float [n_edges] or NULL (meaning 1), both by position in the
 * destination-ordered list.  Replica k reads hidden rows k * n_src + s and a_s rows k * n_src + s (hidden [n_rep * n_src, ld], a_s
 * [n_rep * n_src, ap]) and writes agg_out rows k * n_dst + o ([n_rep * n_dst, ld]) and alpha_out[k * n_edges + e] ([n_rep * n_edges] or
 * NULL); rela, a_r, a_q, w_alpha, b_alpha and every index array are shared by the replicas.
 *   g       = fmaf(t[k], gate_hi[e] - gate_lo[e], gate_lo[e])      lo == hi: that value exactly; lo = 0, hi = 1, t = 1: exactly 1
 *   alpha_e   as rg_digraph_layer_fwd forms it from the replica's a_s row: the gate does not enter it
 *   c       = g * alpha_e, rounded once;   acc = fmaf(c, hidden[s] + rela[r], acc) in list order
 * At g == 1 every bit is rg_digraph_layer_fwd's.  A work item is a (replica, destination or chunk) pair, so a replica's outputs have
 * the bits of an n_rep = 1 call with that replica's t, whatever else the call carries; no float atomics.  scratch:
 * rg_digraph_layer_fwd_gated_scratch_bytes(dst_ptr_host, n_dst, ld, n_rep) bytes (the chunk list once, partial rows per replica).
 * Errors, all before anything is enqueued: n_rep < 1 or > 65535; n_rep * max(n_src, n_dst), n_rep * n_edges or n_rep * (n_dst +
 * chunks) beyond int32; a NULL t; and rg_digraph_layer_fwd's. */
size_t rg_digraph_layer_fwd_gated_scratch_bytes(const int32_t* dst_ptr_host, int32_t n_dst, int32_t ld, int32_t n_rep);
int rg_digraph_layer_fwd_gated(int32_t n_rep, const float* t, const float* gate_lo, const float* gate_hi, int32_t n_dst, int64_t n_edges,
                               const int32_t* dst_ptr, const int32_t* dst_ptr_host, const int32_t* src_idx, const int32_t* rel,
                               const int32_t* row_of_dst, int32_t n_src, int32_t n_rela_rows, int32_t batch, const float* hidden,
                               const float* rela, int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                               const float* w_alpha, const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out,
                               void* scratch, size_t scratch_bytes, void* stream);

/* ---- ... and its adjoint: rg_digraph_layer_bwd at the gates g above, for the same n_rep replicas (static form only).  Everything
 * rg_digraph_layer_bwd states holds, plus t, gate_lo and gate_hi as in rg_digraph_layer_fwd_gated.  Replica k reads hidden rows
 * k * n_src + s, a_s rows k * n_src + s and G = grad_agg rows k * n_dst + o ([n_rep * n_dst, ld]); the source view (src_ptr, edge_of,
 * dst_of_edge), rel, row_of_dst and the constant tables are shared.  With c = g * alpha_e as the forward rounds it:
 *   grad_gate[k * n_edges + e]  = alpha_e * <G[o], hidden[s] + rela[r]>                 [n_rep * n_edges]: the derivative with respect to
 *                                                                                     g itself; the gate does not scale it
 *   grad_hidden[k * n_src + s] += c * G[o]                                             [n_rep * n_src, ld]
 *   grad_a_s[k * n_src + s]    += g * (g_alpha * alpha_e * (1 - alpha_e)) * w * 1[pre > 0]      [n_rep * n_src, ap]
 * the products arranged so that g == 1 leaves rg_digraph_layer_bwd's bits.  A work item is a (replica, source or chunk) pair: a
 * replica's outputs have the bits of an n_rep = 1 call with its t.  scratch: rg_digraph_layer_bwd_gated_scratch_bytes(src_ptr_host,
 * n_src, ld, ap, n_rep) bytes.  The same errors as the gated forward's, before anything is enqueued. */
size_t rg_digraph_layer_bwd_gated_scratch_bytes(const int32_t* src_ptr_host, int32_t n_src, int32_t ld, int32_t ap, int32_t n_rep);
int rg_digraph_layer_bwd_gated(int32_t n_rep, const float* t, const float* gate_lo, const float* gate_hi, int32_t n_src, int32_t n_dst,
                               int64_t n_edges, const int32_t* src_ptr, const int32_t* src_ptr_host, const int32_t* edge_of,
                               const int32_t* dst_of_edge, const int32_t* rel, const int32_t* row_of_dst, int32_t n_rela_rows,
                               int32_t batch, const float* hidden, const float* rela, int32_t d, int32_t ld, const float* a_s,
                               const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                               int32_t attn_dim, const float* grad_agg, float* grad_gate, float* grad_hidden, float* grad_a_s,
                               void* scratch, size_t scratch_bytes, void* stream);

/* ---- ... and both with a gate per (replica, edge) instead of the path lo .. hi (learned edge masks, explain.RDigraph.learn_mask):
 * gate float [n_rep * n_edges] (device), replica k's gate of the edge at list position e being gate[k * n_edges + e], taken as it is.
 * Every other argument is the one of the same name of rg_digraph_layer_fwd_gated / rg_digraph_layer_bwd_gated and everything those two
 * state holds: replica k reads hidden and a_s rows k * n_src + s, the outputs are stacked per replica, the gate does not enter
 * alpha_e, c = g * alpha_e is rounded once, the split rule and the argument checks are the same.  They are the GATED instantiations
 * with a replica stride on the gate pointer, so replica k's outputs (agg_out, alpha_out; grad_gate, grad_hidden, grad_a_s) have the
 * bits of an n_rep = 1 call of the _gated entry point with gate_lo == gate_hi == gate + k * n_edges and t = 1, whatever else the call
 * carries.  scratch: rg_digraph_layer_fwd_gated_scratch_bytes / rg_digraph_layer_bwd_gated_scratch_bytes serve these calls too.  Errors
 * as the _gated calls', with a NULL gate in the place of a NULL t. */
int rg_digraph_layer_fwd_gates(int32_t n_rep, const float* gate, int32_t n_dst, int64_t n_edges, const int32_t* dst_ptr,
                               const int32_t* dst_ptr_host, const int32_t* src_idx, const int32_t* rel, const int32_t* row_of_dst,
                               int32_t n_src, int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela, int32_t d,
                               int32_t ld, const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                               const float* b_alpha, int32_t attn_dim, float* agg_out, float* alpha_out, void* scratch,
                               size_t scratch_bytes, void* stream);
int rg_digraph_layer_bwd_gates(int32_t n_rep, const float* gate, int32_t n_src, int32_t n_dst, int64_t n_edges, const int32_t* src_ptr,
                               const int32_t* src_ptr_host, const int32_t* edge_of, const int32_t* dst_of_edge, const int32_t* rel,
                               const int32_t* row_of_dst, int32_t n_rela_rows, int32_t batch, const float* hidden, const float* rela,
                               int32_t d, int32_t ld, const float* a_s, const float* a_r, const float* a_q, int32_t ap,
                               const float* w_alpha, const float* b_alpha, int32_t attn_dim, const float* grad_agg, float* grad_gate,
                               float* grad_hidden, float* grad_a_s, void* scratch, size_t scratch_bytes, void* stream);

/* ---- one step of learning an edge mask (csrc/mask_step.hip; explain.RDigraph.learn_mask): the objective's chain rule, the
 * regularisers, Adam and the new gate for n_rep replicas of a digraph's n_edges edges, all arrays on the device.  The edges are
 * ordered by row, offsets int64 [batch + 1] the digraph's own (clamped into 0 .. n_edges); free_edge uint8 [n_edges] marks the edges
 * that are learned.  Per replica k and row b: score float [n_rep * batch] the current score, target / inv_scale / inv_n float [batch]
 * (inv_n = 1 / the row's free edges, or 0), lambda_size / lambda_ent float [n_rep], grad float [n_rep * n_edges] = d score / d gate.
 *   L[k, b] = ((score - target) inv_scale)^2 + lambda_size[k] inv_n[b] sum_e g_e + lambda_ent[k] sum_e H(g_e),  g = 1 / (1 + expf(-theta))
 * For every free edge e of row b, t = step >= 1:
 *   dL/dg = 2 (score[k, b] - target[b]) inv_scale[b]^2 grad[k, e] + lambda_size[k] inv_n[b] - lambda_ent[k] theta       (dH/dg = -theta)
 *   gt = dL/dg g (1 - g);   m' = beta1 m + (1 - beta1) gt;   v' = beta2 v + (1 - beta2) gt^2
 *   theta' = theta - lr (m' / (1 - beta1^t)) / (sqrtf(v' / (1 - beta2^t)) + eps);   gate_out[k, e] = 1 / (1 + expf(-theta'))
 * theta, m, v float [n_rep * n_edges] are updated in place, gate_out float [n_rep * n_edges] is written; an edge that is not free
 * keeps all four, bit for bit.  size_out float [n_rep * batch] = the sum of gate_out over the row's free edges, count_out int32
 * [n_rep * batch] = how many of them are > 0.5.  No float atomics: a row is cut into chunks of RG_MASK_CHUNK edges counted from its
 * own first edge, a chunk is summed in a fixed order and the chunks are added in chunk order, so every output has the same bits on
 * every run and replica k's are those of an n_rep = 1 call on its slices.  No scratch.  Errors, all before anything is enqueued:
 * n_rep < 1, step < 1, a negative size, beta1 or beta2 outside [0, 1), a NULL array, n_rep * n_edges or n_rep * batch beyond int32.
 * n_edges == 0 or batch == 0 succeeds and launches nothing. */
#define RG_MASK_CHUNK 512
int rg_mask_step(int32_t n_rep, int32_t batch, int64_t n_edges, const int64_t* offsets, const uint8_t* free_edge, const float* score,
                 const float* target, const float* inv_scale, const float* inv_n, const float* lambda_size, const float* lambda_ent,
                 const float* grad, float lr, float beta1, float beta2, float eps, int32_t step, float* theta, float* m, float* v,
                 float* gate_out, float* size_out, int32_t* count_out, void* stream);

/* ---- tied edge masks (csrc/mask_tie.hip; explain.RDigraph.learn_tied_mask, explain.learn_mask(tie=)): one learned gate per GROUP of
 * edges - a fact with all its copies, a (hop, relation) pair, any label - every member edge reading its group's gate.  rg_mask_step
 * runs unchanged on the group arrays ([n_rep * n_groups], offsets = the rows' group ranges, free_edge all ones); these two calls are
 * the chain rule through the tie and the way back.  All arrays on the device except grp_ptr_host.
 *
 * rg_mask_tie_grad:  grp_grad[k * n_groups + g] = sum over p in grp_ptr[g] .. grp_ptr[g + 1] of grad[k * n_edges + member[p]]
 * grp_ptr int32 [n_groups + 1] (device) and grp_ptr_host, the same array on the host, for the checks and the chunk list; member int32
 * [n_member] the edges' list positions, a group's members contiguous, each clamped into 0 .. n_edges - 1; grad float
 * [n_rep * n_edges]; grp_grad float [n_rep * n_groups].  The sum is defined, in float:
 *   a group of n members is cut into chunks of RG_MASK_TIE_CHUNK members counted from its own first member;
 *   chunk sum = ((x0 + x1) + x2) + ..., x_i the chunk's values in member order, starting FROM x0 (one member: that value's bits);
 *   group sum = ((c0 + c1) + c2) + ..., the chunk sums in chunk order, starting from c0;   an empty group gives +0.
 * No float atomics: a group of one chunk is summed by one lane, a cut group's chunks by a lane each into partial sums a second launch
 * adds in chunk order, so every output has the same bits on every run, whatever the other groups and replicas are, and replica k's are
 * those of an n_rep = 1 call on its slices.  scratch: rg_mask_tie_grad_scratch_bytes(grp_ptr_host, n_groups, n_rep) bytes, 16-B aligned;
 * 0 (scratch may be NULL) when no group has more than RG_MASK_TIE_CHUNK members.  Errors, all before anything is enqueued: n_rep < 1,
 * a negative size, n_rep * n_edges, n_rep * n_groups, n_rep * (the chunks of all groups) or n_member beyond int32, a NULL array,
 * grp_ptr_host not starting at 0, decreasing or not ending at n_member, members without an edge (n_edges == 0), scratch too small.
 * n_groups == 0 succeeds and launches nothing.
 *
 * rg_mask_tie_gates:  gate_out[k * n_edges + e] = grp_gate[k * n_groups + min(group_of[e], n_groups - 1)]  where group_of[e] >= 0
 * group_of int32 [n_edges], -1 (any negative value): the edge is not tied and its gate_out cell is left as it is - nothing is stored
 * there; grp_gate float [n_rep * n_groups]; gate_out float [n_rep * n_edges].  A copy: the bits are the group's.  Errors: n_rep < 1, a
 * negative size, n_rep * n_edges or n_rep * n_groups beyond int32, a NULL array.  n_edges == 0 or n_groups == 0 succeeds and launches
 * nothing. */
#define RG_MASK_TIE_CHUNK 32
size_t rg_mask_tie_grad_scratch_bytes(const int32_t* grp_ptr_host, int32_t n_groups, int32_t n_rep);
int rg_mask_tie_grad(int32_t n_rep, int64_t n_edges, int32_t n_groups, int64_t n_member, const int32_t* grp_ptr,
                     const int32_t* grp_ptr_host, const int32_t* member, const float* grad, float* grp_grad, void* scratch,
                     size_t scratch_bytes, void* stream);
int rg_mask_tie_gates(int32_t n_rep, int64_t n_edges, int32_t n_groups, const int32_t* group_of, const float* grp_gate, float* gate_out,
                      void* stream);

/* ---- the per-hop index of an edited r-digraph: the arrays rg_digraph_(t)layer_fwd takes, built from the digraph's own edge list
 * under a keep mask (csrc/digraph_index.hip; explain.RDigraph.rescore of an extrapolation digraph).  edges int32 [n_edges, 5] =
 * (row, hop, head, rel, tail) ordered by (row, hop, tail) and offsets int64 [batch + 1] (start at 0, never decrease, end at n_edges:
 * the caller checks that) are DEVICE arrays, as explain returns them; n_edges < 2^31, n_hops in 1..32.
 *
 * rg_digraph_hop_ranges, once per digraph: hop_ptr_out int64 [batch, n_hops + 1] (device), entry (b, l - 1) the first edge of row b
 * with hop >= l and entry (b, n_hops) offsets[b + 1]: one thread per (row, hop), a binary search inside the row's range.  The call
 * waits for the array, copies it to hop_ptr_host (host, same shape) and forms per hop the exclusive scan over the rows of the
 * segment lengths: hop_first_out int32 [n_hops, batch + 1] (device) and hop_edges_host int64 [n_hops] = E_l, the edges of every
 * hop.  Item i of hop l is then edge hop_ptr[b][l - 1] + i - hop_first[l - 1][b] of the row b with hop_first[l - 1][b] <= i <
 * hop_first[l - 1][b + 1].  *status_host: RG_DIGRAPH_INDEX_ROW_HOP when a row's first edge has a hop below 1.  batch == 0 launches
 * nothing.
 *
 * rg_digraph_hop_index, per hop l = `hop`: hop_ptr the array above, hop_first the hop's row of hop_first_out, n_hop_edges = E_l;
 * keep uint8 [n_edges] or NULL (every edge kept); keys_prev int64 [n_prev], sorted and unique, row * n_ent + entity: the nodes one
 * hop down (hop 0: (b, q_sub[b])).  An edge is live iff it is kept, has hop l and its (row, head) is in keys_prev.  Outputs, device
 * arrays the caller owns, sized for E_l (dst_ptr_out for E_l + 1), of which the first n_live / n_dst (+ 1) entries are written:
 *   at_out int32 [n_live]    the live edges' indices, ascending
 *   src_out int32 [n_live]   the position of (row, head) in keys_prev
 *   rel_out int32 [n_live], time_out int32 [n_live] = edge_time[at] (edge_time int32 [n_edges]; both NULL: no times)
 *   keys_out int64 [n_dst]   the hop's nodes, the distinct row * n_ent + tail of the live edges, ascending
 *   dst_ptr_out int32 [n_dst + 1]  the CSR of the live edges by node;  row_of_out int32 [n_dst];  prev_idx_out int32 [n_dst] the
 *                            node's position in keys_prev, -1 where it is new
 *   live uint8 [n_edges]     live[at] = 1, every other byte left as it was
 * exactly what explain._hop_index forms in torch for the same inputs.  One thread per edge of the hop flags and searches,
 * rg::scan_exclusive compacts, the node starts are the places where the compacted list's key changes, a second scan numbers them.
 * *n_live_host, *n_dst_host and *status_host come back in one copy (the call waits for it); status is an OR of
 *   RG_DIGRAPH_INDEX_ORDER      a row's hop-l tails decrease
 *   RG_DIGRAPH_INDEX_TWO_TAILS  hop == n_hops and a row has two nodes
 *   RG_DIGRAPH_INDEX_ROW_HOP    an edge's row is not the row of its range, or its hop is not l
 *   RG_DIGRAPH_INDEX_ENTITY     a head or tail outside 0..n_ent-1
 *   RG_DIGRAPH_INDEX_RELATION   a relation outside 0..n_rela_rows-1
 * over EVERY edge of the hop, kept or not; with a non-zero status the outputs are unspecified (but inside their arrays).  Every index
 * is clamped before it is used as an address: malformed arrays give a status, never a fault.  Integers only; no bit depends on the
 * launch geometry.  scratch: rg_digraph_hop_index_scratch_bytes(n_hop_edges) bytes, 256-B aligned (0: nothing to do, or E_l >= 2^31).
 * n_hop_edges == 0 or n_prev == 0 succeeds with n_live = n_dst = 0 and launches nothing.  Every argument error is reported before
 * anything is enqueued.  Neither call is for stream capture. */
#define RG_DIGRAPH_INDEX_ORDER 1
#define RG_DIGRAPH_INDEX_TWO_TAILS 2
#define RG_DIGRAPH_INDEX_ROW_HOP 4
#define RG_DIGRAPH_INDEX_ENTITY 8
#define RG_DIGRAPH_INDEX_RELATION 16
int rg_digraph_hop_ranges(const int32_t* edges, const int64_t* offsets, int64_t n_edges, int32_t batch, int32_t n_hops,
                          int64_t* hop_ptr_out, int32_t* hop_first_out, int64_t* hop_ptr_host, int64_t* hop_edges_host,
                          int32_t* status_host, void* stream);
size_t rg_digraph_hop_index_scratch_bytes(int64_t n_hop_edges);
int rg_digraph_hop_index(const int32_t* edges, const uint8_t* keep, const int32_t* edge_time, int64_t n_edges, int32_t batch,
                         int32_t n_hops, int32_t hop, const int64_t* hop_ptr, const int32_t* hop_first, int64_t n_hop_edges,
                         const int64_t* keys_prev, int64_t n_prev, int32_t n_ent, int32_t n_rela_rows, int32_t* at_out,
                         int32_t* src_out, int32_t* rel_out, int32_t* time_out, int64_t* keys_out, int32_t* dst_ptr_out,
                         int32_t* row_of_out, int32_t* prev_idx_out, uint8_t* live, void* scratch, size_t scratch_bytes,
                         int64_t* n_live_host, int64_t* n_dst_host, int32_t* status_host, void* stream);

/* ---- rule quality: support and confidence of rules (head h, body r_1..r_L) counted on the whole graph; no counterpart in the
 * reference (its *_rule_vis.py scripts only draw).  The graph is used as built, inverse and identity rows included: for a relation id
 * r in 0..n_rela_rows-1, A_r(x, y) holds iff the graph has at least one row (x, r, y) (a repeated fact counts once), and body(x, y)
 * holds iff there are z_0 = x, .., z_L = y with A_{r_l}(z_{l-1}, z_l) for every l (identity steps are ordinary steps).
 * head int32 [n_rules], body int32 [n_rules, n_hops], sources int32 [n_sources] (distinct entity ids) and counts are DEVICE arrays;
 * n_hops in 1..32, n_rules <= 65535.  counts int64 [n_rules, 4] is ADDED to (caller-zeroed; calls over disjoint source sets sum):
 *   [0] body_pairs      #{(x, y): x a source, body(x, y)}
 *   [1] hits            #{(x, y): x a source, body(x, y) and A_h(x, y)}                 (AMIE's support)
 *   [2] pca_body_pairs  #{(x, y): x a source, body(x, y) and A_h(x, y') for some y'}
 *   [3] head_pairs      #{(x, y): x a source, A_h(x, y)}
 * so hits <= pca_body_pairs <= body_pairs and hits <= head_pairs.  A chain of boolean sparse products on entity-major bitmaps over
 * the sources (csrc/rule_ground.hip): per hop |edges of r_l| * ceil(n_sources / 32) words are read and ORed with integer atomics,
 * then one counting pass; OR and integer adds are order-independent, so every count is exact, the same in every run and the same
 * however the rules and sources are cut into calls.  scratch holds rg_rule_ground_scratch_bytes(n_ent, n_rules, n_sources) bytes
 * (three bitmaps uint32 [n_rules][n_ent][ceil(n_sources / 32)] and one word row per rule; 0: an argument < 1, n_rules > 65535 or
 * more than 2^40 words per bitmap), 4-B aligned, and is zeroed by the call.  Errors: a temporal graph (n_time != 0: temporal rules
 * carry a direction per step and are grounded by rg_trule_ground), a graph without its CSR by relation, n_rules / n_hops /
 * n_sources out of range.  A relation id outside 0..n_rela_rows-1 reads nothing (that rule's body or head is empty) and a source
 * outside 0..n_ent-1 is skipped:
 * nothing outside the graph's arrays or the scratch is touched whatever the id arrays hold; the caller validates them (engine.py).
 * Allocates nothing, asynchronous on `stream`. */
size_t rg_rule_ground_scratch_bytes(int32_t n_ent, int32_t n_rules, int32_t n_sources);
int rg_rule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, int32_t n_rules, int32_t n_hops,
                   const int32_t* sources, int32_t n_sources, void* scratch, int64_t* counts, void* stream);

/* ---- temporal rule quality: rg_rule_ground for the quadruple graph of the interpolation model (n_time != 0); no counterpart in the
 * reference.  A temporal rule is a head relation h and a body of L steps (r_l, d_l); d is the forward's direction of an edge of time id
 * tau against a query time id t (dt = tau - t): 0 past (dt < 0), 1 now (dt == 0), 2 future (dt > 0), and 3 = any edge time.  An anchor
 * is a pair (x, t) of an entity and a query time id.  On the graph as built, rows (head, rel, tail, time) with inverse and identity
 * rows as the caller's quadruples hold them, a repeated row counting once: A_{r,d}(u, v | t) holds iff the graph has a row
 * (u, r, v, tau) whose direction against t is d (any such row if d == 3); body(x, y | t) iff there are z_0 = x, .., z_L = y with
 * A_{r_l,d_l}(z_{l-1}, z_l | t) for every l (identity steps are ordinary steps); head(x, y | t) iff the graph has the row (x, h, y, t):
 * the head is a "now" step.  counts int64 [n_rules, 4] is ADDED to (caller-zeroed; calls over disjoint anchor sets sum):
 *   [0] body_pairs      #{((x, t), y): body(x, y | t)}
 *   [1] hits            #{((x, t), y): body(x, y | t) and head(x, y | t)}
 *   [2] pca_body_pairs  #{((x, t), y): body(x, y | t) and head(x, y' | t) for some y'}
 *   [3] head_pairs      #{((x, t), y): head(x, y | t)}
 * over the anchors of the call, so hits <= pca_body_pairs <= body_pairs and hits <= head_pairs.  head int32 [n_rules], body and dir
 * int32 [n_rules, n_hops] (dir in 0..3); the anchors are j = 0..n_anchors-1, distinct and sorted by time id: anchor_ent int32
 * [n_anchors] holds their entities and anchor_ptr int32 [n_time + 1] the first j whose time is >= tau, anchor_ptr[n_time] = n_anchors,
 * so the times are implied.  All arrays are DEVICE arrays; n_hops in 1..32, n_rules <= 65535.  The bitmaps of rg_rule_ground with
 * anchors for columns (csrc/trule_ground.hip): an edge (u, v, tau) moves one contiguous column range, past [ptr[tau+1], S), now
 * [ptr[tau], ptr[tau+1]), future [0, ptr[tau]), any [0, S); per hop |edges of r_l| * (words in range) words are read, masked and ORed
 * with integer atomics, then one counting pass.  OR and integer adds are order-independent, so every count is exact, the same in every
 * run and the same however the rules and the sorted anchors are cut into calls.  scratch holds rg_trule_ground_scratch_bytes(n_ent,
 * n_rules, n_anchors) bytes (the layout and the 0 cases of rg_rule_ground_scratch_bytes), 4-B aligned, and is zeroed by the call.
 * Errors: a NULL graph, a static graph (n_time == 0: use rg_rule_ground), a graph without its CSR by relation and edge times, n_hops
 * outside 1..32, n_rules > 65535, n_anchors < 0; n_rules == 0 or n_anchors == 0 does nothing.  A relation id outside 0..n_rela_rows-1
 * is tested before any load and reads nothing, a direction outside 0..3 makes the step empty, an edge end or anchor entity outside
 * 0..n_ent-1 and an edge time outside 0..n_time-1 are skipped, anchor_ptr entries are clamped to 0..n_anchors and an empty range moves
 * nothing: nothing outside the graph's arrays or the scratch is touched whatever the id arrays hold; the caller validates them
 * (engine.py).  Allocates nothing, asynchronous on `stream`. */
size_t rg_trule_ground_scratch_bytes(int32_t n_ent, int32_t n_rules, int32_t n_anchors);
int rg_trule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* dir, int32_t n_rules, int32_t n_hops,
                    const int32_t* anchor_ent, const int32_t* anchor_ptr, int32_t n_anchors, void* scratch, int64_t* counts,
                    void* stream);

/* ---- extrapolation rule quality: rg_rule_ground for the one-graph layout of the forecasting model (extrapolation.T_RED_GNN); no
 * counterpart in the reference.  The model's data: data[j] = (s, r, o, ts), j = 0..n_data-1, sorted by time; row_day[j] = ts //
 * time_granularity; off = the model's time_offset_list, n_day = len(off); a query day t has the forward's row window [win_lo[t],
 * win_hi[t]) = [off[max(t - 120, 0)], off[t]).  The window keeps the reference's quirks: off[t] is the index of the LAST row of day
 * t - 1, so that row is left out, and off[t] is 0 after a day without rows, so a window is empty or reaches back to row 0.  The windows
 * are therefore NOT monotone in t, and rows with a lag far above 120 occur.
 * An extrapolation rule is a head relation h and L steps (r_l, [lag_lo_l, lag_hi_l)): every edge of the forecasting model lies in the
 * past, so what tells one step from another is how far back the fact lies.  An anchor is a pair (x, t) of an entity and a query day.
 * The graph is used as T_RED_GNN builds it: the self-loops first, relation id n_rel_true and time field n_data, then the data rows, each
 * with its own row index as time field (g->n_time == n_data + 1).  A step (r, [lo, hi)) admits the data row j = (u, r, v) at day t iff
 * win_lo[t] <= j < win_hi[t] and lo <= t - row_day[j] < hi; it admits the self-loop (u, n_rel_true, u) at day t iff lo <=
 * min(t, loop_window) < hi, the lag the forward gives the self-loop (loop_window = 120).  "Any lag" is [0, INT32_MAX): every self-loop
 * and every data row of the window.  body(x, y | t) holds iff there are z_0 = x, .., z_L = y with an admitted row (z_{l-1}, r_l, z_l)
 * for every l (a repeated row counts once: the products are boolean); head(x, y | t) iff some data row (x, h, y) has row_day == t -
 * the fact on the query day itself, which no window holds; a self-loop is never a head.  counts int64 [n_rules, 4] is ADDED to
 * (caller-zeroed; calls over disjoint anchor sets sum), its columns body_pairs, hits, pca_body_pairs, head_pairs over ((x, t), y)
 * exactly as rg_trule_ground defines them, so hits <= pca_body_pairs <= body_pairs and hits <= head_pairs.
 * head int32 [n_rules]; body, lag_lo and lag_hi int32 [n_rules, n_hops]; row_day int32 [n_data]; win_lo and win_hi int32 [n_day]; the
 * anchors are j = 0..n_anchors-1, distinct and sorted by day: anchor_ent int32 [n_anchors] holds their entities and anchor_ptr int32
 * [n_day + 1] the first j whose day is >= t.  All arrays are DEVICE arrays; n_hops in 1..32, n_rules <= 65535.  The bitmaps of
 * rg_rule_ground with anchors for columns (csrc/xrule_ground.hip): an edge walks its step's candidate days, [row_day[j] + lag_lo,
 * min(row_day[j] + lag_hi, n_day)) for a data row (each day tested against its window), one range of days for a self-loop, and every
 * run of consecutive passing days [a, b) moves the columns [anchor_ptr[a], anchor_ptr[b]), masked at both end words and ORed with
 * integer atomics; the head pass moves the columns of day row_day[j] without a window test; then one counting pass.  OR and integer
 * adds are order-independent, so every count is exact, the same in every run and the same however the rules and the sorted anchors
 * are cut into calls.  scratch holds rg_rule_ground_scratch_bytes(n_ent, n_rules, n_anchors) bytes (that layout), 4-B aligned, and is
 * zeroed by the call.  Errors: a NULL graph, a graph that is not the extrapolation layout (n_time != n_data + 1, or no CSR by relation
 * with edge times), n_hops outside 1..32, n_rules > 65535, n_anchors < 0, n_day < 1, loop_window < 0; n_rules == 0 or n_anchors == 0
 * does nothing.  A relation id outside 0..n_rela_rows-1 is tested before any load and reads nothing, lag_lo >= lag_hi makes the step
 * empty, an edge end or anchor entity outside 0..n_ent-1, a row index outside 0..n_data and a row_day outside 0..n_day-1 are skipped,
 * the days are formed in 64 bits and clamped to 0..n_day, anchor_ptr entries are clamped to 0..n_anchors and an empty range moves
 * nothing: nothing outside the graph's arrays, row_day[0..n_data), win_lo / win_hi[0..n_day), the anchor arrays, the scratch and
 * counts is touched whatever the id arrays hold; the caller validates them (engine.py).  Allocates nothing, asynchronous on `stream`. */
int rg_xrule_ground(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* lag_lo, const int32_t* lag_hi,
                    int32_t n_rules, int32_t n_hops, const int32_t* row_day, int32_t n_data,
                    const int32_t* win_lo, const int32_t* win_hi, int32_t n_day, int32_t loop_window,
                    const int32_t* anchor_ent, const int32_t* anchor_ptr, int32_t n_anchors,
                    void* scratch, int64_t* counts, void* stream);

/* ---- rule application: which answers weighted rules predict for queries (s, r, ?), and which rule is behind each; no counterpart in
 * the reference.  The graph, A_r(x, y) and body(x, y) are exactly those of rg_rule_ground.  The rules are (head[i], body[i][0..L-1],
 * weight[i]), i = 0..n_rules-1, head non-decreasing, weight fp32 in (0, 1] and miss[i] = fl32(1 - weight[i]) formed by the caller (in
 * the kernel the compiler could contract surv * (1 - w) into one rounding).  The queries are (sub[b], rel[b]), b = 0..batch-1,
 * duplicates allowed, given sorted by relation (stably): q_sub int32 [batch] the subjects in sorted order, q_row int32 [batch] the
 * caller's row b of each sorted position, q_ptr int32 [n_rela_rows + 1] with the sorted positions of relation r = q_ptr[r]..q_ptr[r+1].
 * Rule i fires for cell (b, y) iff head[i] == rel[b] and body_i(sub[b], y).  The four outputs, fp32 / fp32 / int32 / int32
 * [batch, n_ent] with row stride n_ent, are initialised by the caller (best = 0, surv = 1, best_rule = -1, fired = 0 before the first
 * rule) and carried through: per cell the rules that fire are visited in ascending i,
 *   fired += 1;  surv = fl32(surv * miss[i]);  if (weight[i] > best) { best = weight[i]; best_rule = rule_base + i; }
 * (strict: the first of equal weights wins).  "max" aggregation is best, noisy-or is fl32(1 - surv), taken by the caller.  Only the
 * order of i matters: every output is the same bit for bit in every run and however the rules are cut into consecutive calls on one
 * stream (rule_base = the first rule's index in the whole list).
 * Rule i has S_i = q_ptr[h+1] - q_ptr[h] sources (h = head[i]), W_i = ceil(S_i / 32) words per entity, and two bitmaps that are slabs
 * of n_ent * W_i words starting at word slab[i] of the two halves of the scratch; slab int64 [n_rules + 1] is the exclusive prefix of
 * n_ent * W_i, computed by the caller, n_words = slab[n_rules], and scratch holds rg_rule_apply_scratch_bytes(n_words) bytes (0:
 * n_words < 1 or > 2^40), 4-B aligned.  phases: 1 = zero the scratch, seed and hop (leaves the bitmaps in the scratch), 2 = aggregate
 * from them, 3 = both (a timing probe issues them apart).  All arrays are DEVICE arrays.  Errors: a NULL or temporal graph (as
 * rg_rule_ground), a graph without its CSR by relation, n_hops outside 1..32, n_rules > 65535, n_words out of range.  A relation id
 * outside 0..n_rela_rows-1 is tested before any load and reads nothing, an edge end or subject outside 0..n_ent-1 and a q_row outside
 * 0..batch-1 are skipped, q_ptr entries are clamped to 0..batch, a slab outside 0..n_words is left out; an unsorted head makes the
 * result unspecified: nothing outside the graph's arrays, the scratch or the four outputs is touched whatever the arrays hold; the
 * caller validates them (engine.py).  Allocates nothing, asynchronous on `stream`. */
size_t rg_rule_apply_scratch_bytes(int64_t n_words);
int rg_rule_apply(const rg_graph* g, const int32_t* head, const int32_t* body, const float* weight, const float* miss,
                  int32_t n_rules, int32_t n_hops, int32_t rule_base, const int32_t* q_sub, const int32_t* q_row,
                  const int32_t* q_ptr, int32_t batch, const int64_t* slab, int64_t n_words, void* scratch, int32_t phases,
                  float* best, float* surv, int32_t* best_rule, int32_t* fired, void* stream);

/* ---- temporal rule application: rg_rule_apply for the quadruple graph of the interpolation model (n_time != 0): which answers
 * weighted temporal rules predict for queries (s, r, ?, t), and which rule is behind each; no counterpart in the reference.  The graph,
 * the directions and body(x, y | t) are exactly those of rg_trule_ground: a step (r, d) admits a row (u, r, v, tau) for a query of time
 * id t iff d == 3, or the forward's direction of tau - t is d (0 past, 1 now, 2 future); identity steps are ordinary steps.  The rules
 * are (head[i], body[i][0..L-1], dir[i][0..L-1], weight[i]), i = 0..n_rules-1, head non-decreasing, weight fp32 in (0, 1] and miss[i] =
 * fl32(1 - weight[i]) formed by the caller.  The queries are (sub[b], rel[b], time[b]), b = 0..batch-1, duplicates allowed.  Rule i
 * fires for cell (b, y) iff head[i] == rel[b] and body_i(sub[b], y | time[b]).  The four outputs, fp32 / fp32 / int32 / int32
 * [batch, n_ent] with row stride n_ent, are initialised by the caller (0 / 1 / -1 / 0) and folded exactly as in rg_rule_apply, in
 * ascending i:
 *   fired += 1;  surv = fl32(surv * miss[i]);  if (weight[i] > best) { best = weight[i]; best_rule = rule_base + i; }
 * Every output is the same bit for bit in every run, for every grid and lane-group choice, and however the rules are cut into
 * consecutive calls on one stream.
 * The queries are given sorted stably by the key rel * n_time + time: q_sub int32 [batch] the subjects and q_row int32 [batch] the
 * caller's row b, both in sorted order, and q_ptr int32 [n_rela_rows * n_time + 1], q_ptr[k] the first sorted position whose key is
 * >= k (the last entry = batch).  Relation h owns the positions p0 = q_ptr[h * n_time] .. p1 = q_ptr[(h + 1) * n_time]: rule i of head
 * h has S_i = p1 - p0 sources, W_i = ceil(S_i / 32) words per entity and two slabs of n_ent * W_i words at word slab[i] of the two
 * halves of the scratch, slab int64 [n_rules + 1], n_words = slab[n_rules], scratch of rg_rule_apply_scratch_bytes(n_words) bytes -
 * all as in rg_rule_apply.  Query times are never loaded: for an edge (u, v, tau) of the step's relation the columns it may move are
 * now [q_ptr[h * n_time + tau] - p0, q_ptr[h * n_time + tau + 1] - p0), past from that upper bound to S_i, future from 0 to that lower
 * bound, any [0, S_i); per hop |edges of r_l| * (words in range) words are read, masked at both ends and ORed with integer atomics
 * (csrc/trule_apply.hip).  phases: 1 = zero the scratch, seed and hop, 2 = aggregate, 3 = both.  All arrays are DEVICE arrays; n_hops
 * in 1..32, n_rules <= 65535.  Errors: a NULL graph, a static graph (n_time == 0: use rg_rule_apply), a graph without its CSR by
 * relation and edge times, n_rules / n_hops / batch / phases / rule_base / n_words out of range; n_rules == 0 or batch == 0 does
 * nothing.  A relation id outside 0..n_rela_rows-1 is tested before any load and reads nothing, a direction outside 0..3 makes the step
 * empty, an edge end or subject outside 0..n_ent-1, an edge time outside 0..n_time-1 and a q_row outside 0..batch-1 are skipped, q_ptr
 * is indexed in int64 and its entries are clamped to 0..batch, a slab outside 0..n_words is left out and an empty range moves nothing;
 * an unsorted head makes the result unspecified: nothing outside the graph's arrays, the scratch or the four outputs is touched
 * whatever the arrays hold; the caller validates them (engine.py).  Allocates nothing, asynchronous on `stream`. */
int rg_trule_apply(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* dir, const float* weight,
                   const float* miss, int32_t n_rules, int32_t n_hops, int32_t rule_base, const int32_t* q_sub, const int32_t* q_row,
                   const int32_t* q_ptr, int32_t batch, const int64_t* slab, int64_t n_words, void* scratch, int32_t phases,
                   float* best, float* surv, int32_t* best_rule, int32_t* fired, void* stream);

/* ---- extrapolation rule application: rg_rule_apply for the one-graph layout of the forecasting model (extrapolation.T_RED_GNN): which
 * answers weighted extrapolation rules forecast for queries (s, r, ?, day t), and which rule is behind each; no counterpart in the
 * reference.  The graph, row_day, the windows and loop_window are exactly those of rg_xrule_ground, and a step admits an edge for a
 * query of day t exactly as rg_xrule_ground admits it for an anchor of day t: a step (r, [lo, hi)) admits the data row j = (u, r, v)
 * iff win_lo[t] <= j < win_hi[t] and lo <= t - row_day[j] < hi, and the self-loop (u, n_rel_true, u) iff lo <= min(t, loop_window) <
 * hi.  The rules are (head[i], (body[i][l], [lag_lo[i][l], lag_hi[i][l])), weight[i]), i = 0..n_rules-1, l = 0..n_hops-1, head
 * non-decreasing, weight fp32 in (0, 1] and miss[i] = fl32(1 - weight[i]) formed by the caller.  The queries are (sub[b], rel[b],
 * day[b]), b = 0..batch-1, duplicates allowed.  Rule i fires for cell (b, y) iff head[i] == rel[b] and there are z_0 = sub[b], ..,
 * z_L = y with a row (z_{l-1}, body[i][l], z_l) that step l admits for day[b], for every l (a repeated row counts once: the products
 * are boolean).  There is no head pass.  The four outputs, fp32 / fp32 / int32 / int32 [batch, n_ent] with row stride n_ent, are
 * initialised by the caller (0 / 1 / -1 / 0) and folded exactly as in rg_rule_apply, in ascending i:
 *   fired += 1;  surv = fl32(surv * miss[i]);  if (weight[i] > best) { best = weight[i]; best_rule = rule_base + i; }
 * Every output is the same bit for bit in every run, for every grid and lane-group choice, and however the rules are cut into
 * consecutive calls on one stream.
 * The queries are given sorted stably by (rel, day): q_sub int32 [batch] the subjects and q_row int32 [batch] the caller's row b, both
 * in sorted order, and q_ptr int32 [n_rela_rows + 1] with the sorted positions of relation h = q_ptr[h]..q_ptr[h + 1], one entry per
 * relation as in rg_rule_apply; S_i, W_i, slab int64 [n_rules + 1], n_words = slab[n_rules] and the scratch of
 * rg_rule_apply_scratch_bytes(n_words) bytes are that function's too.  The distinct query days of every relation are the "entries":
 * day_ptr int32 [n_rela_rows + 1] - relation h owns the entries day_ptr[h]..day_ptr[h + 1] -, day_of int32 [n_qdays] the day of every
 * entry, ascending inside a relation, and day_pos int32 [n_qdays + 1] the first sorted position of every entry, day_pos[n_qdays] =
 * batch.  Entry k of relation h owns the columns [day_pos[k] - q_ptr[h], day_pos[k + 1] - q_ptr[h]) of the rule's slab.  For a data
 * row j the hop finds the first entry whose day is >= row_day[j] + lag_lo by binary search, walks the entries while their day is below
 * min(row_day[j] + lag_hi, n_day), tests each entry's day against its window and moves every run of consecutive passing entries as one
 * column range, masked at both end words and ORed with integer atomics; a self-loop's days are one range found by two binary searches
 * (csrc/xrule_apply.hip).  Per edge that is O(log entries + entries in range), whatever n_day is.  phases: 1 = zero the scratch, seed
 * and hop, 2 = aggregate, 3 = both.  All arrays are DEVICE arrays; n_hops in 1..32, n_rules <= 65535.  Errors: a NULL graph, a graph
 * that is not the extrapolation layout (n_time != n_data + 1, or no CSR by relation with edge times), n_rules / n_hops / batch / phases
 * / rule_base / n_words out of range, n_day < 1, loop_window < 0, n_qdays < 0, a NULL array; n_rules == 0 or batch == 0 does nothing.
 * A relation id outside 0..n_rela_rows-1 is tested before any load and reads nothing, lag_lo >= lag_hi makes the step empty, an edge
 * end or subject outside 0..n_ent-1, a row index outside 0..n_data, a row_day or day_of value outside 0..n_day-1 and a q_row outside
 * 0..batch-1 are skipped, the candidate days are formed in 64 bits and clamped to 0..n_day, day_ptr entries are clamped to 0..n_qdays,
 * day_pos and q_ptr entries to 0..batch and every range to 0..S_i, an empty range moves nothing and a slab outside 0..n_words is left
 * out; an unsorted head or day_of makes the result of the rules concerned unspecified: nothing outside the graph's arrays,
 * row_day[0..n_data), win_lo / win_hi[0..n_day), the query arrays, the scratch or the four outputs is touched whatever the arrays
 * hold; the caller validates them (engine.py).  Allocates nothing, asynchronous on `stream`. */
int rg_xrule_apply(const rg_graph* g, const int32_t* head, const int32_t* body, const int32_t* lag_lo, const int32_t* lag_hi,
                   const float* weight, const float* miss, int32_t n_rules, int32_t n_hops, int32_t rule_base,
                   const int32_t* row_day, int32_t n_data, const int32_t* win_lo, const int32_t* win_hi, int32_t n_day,
                   int32_t loop_window, const int32_t* q_sub, const int32_t* q_row, const int32_t* q_ptr,
                   const int32_t* day_ptr, const int32_t* day_of, const int32_t* day_pos, int32_t n_qdays, int32_t batch,
                   const int64_t* slab, int64_t n_words, void* scratch, int32_t phases,
                   float* best, float* surv, int32_t* best_rule, int32_t* fired, void* stream);

/* rg_dense_fwd with the node count read on the device (after rg_frontier_expand_async): n_cap = capacity of the row buffers,
 * n_dev = rg_frontier_count_ptr() of the frontier whose newest level the rows belong to, n_hint = the row count the caller expects
 * (0 = unknown): it only sizes the grid, every row count up to n_cap is processed correctly. */
int rg_dense_fwd_dev(int64_t n_cap, const int32_t* n_dev, int64_t n_hint, int32_t d, int32_t ld, const float* agg, const float* hidden_prev,
                     const int32_t* prev_idx, const float* W_h, int32_t act,
                     const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                     const float* Ws_next, int32_t attn_dim, int32_t ap, float* a_s_out,
                     const float* W_final, const int32_t* nodes, int32_t n_ent, float* scores_all,
                     float* hidden_out, int32_t precision, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- dense step of a layer in training: models.py:41 (W_h + act), :81 (h0 carry), :82 (dropout, as a given mask: 0 or
 * 1/(1-p) per element, or NULL), :83 (single-step GRU) in one f32-MFMA kernel that also leaves what the backward pass needs:
 * x_out [n,d] = the GRU input, and gates_ws_out [n,5,d] = {r, z, n, h0, W_hn h0 + b_hn}, the workspace layout of PyTorch's fused
 * GRU cell (so its fused backward kernel applies).  d in 16..64 (multiple of 4) or 128; rows are d floats wide (no padding). */
int rg_dense_train_fwd(int64_t n, int32_t d, const float* agg, const float* hidden_prev, const int32_t* prev_idx,
                       const float* W_h, int32_t act, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                       const float* mask, float* hidden_out, float* x_out, float* gates_ws_out, void* stream);

/* rg_dense_train_fwd that also emits the NEXT layer's hoisted attention projection of the new state, as rg_dense_fwd does in inference:
 * a_s_out [n, ap] = hidden_out Ws_next^T (Ws_next [attn_dim, d], models.py:16,33; columns attn_dim .. ap - 1 are zero; attn_dim <= 16,
 * ap = attn_dim rounded up to a multiple of 4). */
int rg_dense_train_fwd_as(int64_t n, int32_t d, const float* agg, const float* hidden_prev, const int32_t* prev_idx,
                          const float* W_h, int32_t act, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                          const float* mask, const float* Ws_next, int32_t attn_dim, int32_t ap,
                          float* hidden_out, float* x_out, float* gates_ws_out, float* a_s_out, void* stream);

/* out[r, :n] = base[r, :n] + g[r, :k] W[:k, :n] for n_rows node rows (row strides ldb / ldg / ldo in floats): the new state's gradient
 * through a_s = hidden Ws_attn^T added to the gradient it already carries (autograd of models.py:33).  k <= 32, n <= 128, n % 4 == 0;
 * out may alias base. */
int rg_rows_addmm(const float* base, int64_t ldb, const float* g, int64_t ldg, int32_t k, const float* W, int32_t n, int64_t n_rows,
                  float* out, int64_t ldo, void* stream);

/* out[r, :n] = x[r, :k] W^T (+ bias[:n] when bias is non-NULL) for n_rows node rows: W device float [n][k] (a linear layer's weight),
 * row strides ldx >= k and ldo >= n in floats.  Every output element is one fmaf chain over k = 0..k-1 in order, so a row's result does
 * not depend on the number of rows of the call (a GEMM library picks its kernel, and its order of additions, by the shape): the
 * extrapolation model's inference forward uses it so that a query computes the same bits in every batch.  1 <= k <= 4096, n >= 1;
 * columns are tiled so that a tile's weights fit 64 KB of LDS.  Allocates nothing, asynchronous on `stream`. */
int rg_rows_linear(const float* x, int64_t n_rows, int64_t ldx, int32_t k, const float* w, const float* bias, int32_t n,
                   float* out, int64_t ldo, void* stream);

/* Adjoint of rg_dense_train_fwd for the node-row quantities (autograd of models.py:41,81-83): from grad_hidden [n,d] and the saved
 * x / gates_ws (/ mask, keep = 1 - p) it writes grad_gates_i, grad_gates_h [n,3d] (GRU pre-activation gradients, for the weight and
 * bias gradients the caller forms), grad_pre [n,d] (gradient at W_h's output, for dW_h), grad_agg [n,d] and grad_h0 [n,d] (the
 * carried state's gradient, to be gathered back to the previous frontier by old_nodes_new_idx).  d in 16..64, multiple of 4. */
int rg_dense_train_bwd(int64_t n, int32_t d, const float* grad_hidden, const float* gates_ws, const float* x, const float* mask,
                       float keep, int32_t act, const float* W_h, const float* w_ih, const float* w_hh,
                       float* grad_gates_i, float* grad_gates_h, float* grad_pre, float* grad_agg, float* grad_h0, void* stream);

/* rg_dense_train_bwd with two fewer passes over memory: grad_gates_hn [n,d] is only the n-gate block of the hidden-side gate gradients
 * (their r and z blocks equal grad_gates_i's), and with prev_idx [n] (a node's row in the previous frontier or -1: rg_frontier_nodes)
 * the carried state's gradient goes straight to grad_prev [n_old,d] (every row written exactly once; autograd of models.py:81's
 * index_copy); prev_idx NULL: grad_prev is [n,d] = grad_h0. */
int rg_dense_train_bwd2(int64_t n, int32_t d, const float* grad_hidden, const float* gates_ws, const float* x, const float* mask,
                        float keep, int32_t act, const float* W_h, const float* w_ih, const float* w_hh, const int32_t* prev_idx,
                        float* grad_gates_i, float* grad_gates_hn, float* grad_pre, float* grad_agg, float* grad_prev, void* stream);

/* ---- relational digraph of an answer (the r-digraph RED-GNN is named for; the reference draws it per setting with
 * the temporal model_cuda*_vis.py scripts): for row b = (s, r, o) of a batch, the union of the length-L paths s -> o through the frontier's
 * levels (identity edges count as steps), each edge with the attention alpha of its layer (rg_layer_fwd's formula and arithmetic).
 * Needs a frontier that still holds levels 0..L (n_levels >= L + 1) and, per hop l, the arguments rg_layer_fwd had: a_s of level
 * l-1 [N_{l-1}, ap], a_r [2R+1, ap], a_q [B, ap], w_alpha, b_alpha.  Marks are batch-major bitmaps uint32 [batch][ceil(n_ent/32)].
 * rg_explain_seed: marks_out = {(b, objs[b])} where objs[b] is in level `level` (= L); reached_out uint8 [batch] says which.
 * Then for l = L..1:
 * rg_explain_count: the hop-l edges (h, rel, t) with t marked, h in level l-1 and alpha >= min_alpha; marks_prev_out = their heads
 *   (written, every word); word_ptr_out int32 [batch*ceil(n_ent/32) + 1] = exclusive scan of the kept edges per mark word, total
 *   last.  Returns the hop's total in *n_edges_host (synchronises `stream`; < 2^31 per hop).  scratch: rg_explain_scratch_bytes(),
 *   256-B aligned.
 * rg_explain_emit: the same edges, edges_out int32 [E_l, 4] = (row, head, rel, tail) (16-B aligned) and alpha_out [E_l], in
 *   (row, tail, CSR-by-tail position) order, i.e. fact-row order inside a tail; deterministic.
 * rg_explain_gather: puts one hop's list (n edges, `hop` = l) into a (row, hop, ...) layout: edge i of row b goes to
 *   row_base[b] + i - row_first[b] (int64 [batch] each), as (row, hop, head, rel, tail) into edges_out int32 [n_out, 5] and alpha_out.
 * Reads no buffer of the subgraph's edge count: per hop the marked tails' CSR rows, the level bitmap and the attention tables. */
size_t rg_explain_scratch_bytes(const rg_frontier* f);
int rg_explain_seed(const rg_frontier* f, int32_t batch, int32_t n_ent, int32_t level, const int32_t* objs, uint32_t* marks_out,
                    uint8_t* reached_out, void* stream);
int rg_explain_count(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                     int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
                     size_t scratch_bytes, int64_t* n_edges_host, void* stream);
int rg_explain_emit(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                    const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                    int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out, void* stream);
int rg_explain_gather(int64_t n, int32_t hop, int32_t batch, const int32_t* edges, const float* alpha, const int64_t* row_first,
                      const int64_t* row_base, int64_t n_out, int32_t* edges_out, float* alpha_out, void* stream);

/* ---- the same for a temporal graph (T-RED-GNN interpolation; the reference draws this digraph in
 * Temporal/interpolation/model_cuda_rule_vis.py): one hop of the r-digraph over a quadruple graph (rg_tgraph_create).  Arguments,
 * marking walk, scratch, output order and determinism are rg_explain_count / rg_explain_emit's; a_r has n_rela_rows rows and alpha is
 * rg_tlayer_fwd's (which does not read the edge's time; pass b_alpha = 0).  rg_texplain_emit also writes time_out int32 [E_l]: the time
 * id of every kept edge (the CSR-by-tail entry's), so that a fact repeated at several times gives one edge per time, in CSR order.
 * The graph must be temporal (n_time > 0) and the frontier must have no window set (rg_frontier_set_window: that is
 * rg_xexplain_*, below); a static graph, like a temporal one handed to the static entry points, is an argument error.  rg_explain_seed,
 * rg_explain_gather and rg_explain_scratch_bytes serve both settings. */
int rg_texplain_count(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                      const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                      int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
                      size_t scratch_bytes, int64_t* n_edges_host, void* stream);
int rg_texplain_emit(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                     int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out,
                     int32_t* time_out, void* stream);

/* ---- the same for the extrapolation model (extrapolation.py: ONE quadruple graph whose time field is the edge's data row, self-loops
 * row >= n_data, and per-query row windows on the frontier).  The marking walk of rg_explain_count / rg_explain_emit with the forward's
 * window test in both passes: an edge counts for query b only if its row is a self-loop or win_lo[b] <= row < win_hi[b] (rg_xlayer_fwd).
 * alpha is rg_xlayer_fwd's (a_s / a_r / a_q of [h_s | rel | rel_q], no time; pass b_alpha = 0).  rg_xexplain_emit also writes row_out
 * int32 [E_l]: the data row of every kept edge (>= n_data for a self-loop).  The frontier must have its windows set
 * (rg_frontier_set_window; n_data is taken from it) and the graph must carry row ids (rg_tgraph_create).  Arguments, scratch, output
 * order and determinism as rg_explain_count / rg_explain_emit; rg_explain_seed and rg_explain_gather serve this setting too. */
int rg_xexplain_count(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                      const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                      int32_t attn_dim, float min_alpha, uint32_t* marks_prev_out, int32_t* word_ptr_out, void* scratch,
                      size_t scratch_bytes, int64_t* n_edges_host, void* stream);
int rg_xexplain_emit(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, const uint32_t* marks,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                     int32_t attn_dim, float min_alpha, const int32_t* word_ptr, int32_t* edges_out, float* alpha_out,
                     int32_t* row_out, void* stream);

/* ---- attention profile of a hop: which edge relations a query listens to (the reference's attention_vis table,
 * Temporal/interpolation/model_cuda.py:117-119,163-166: per relation the sum of alpha and the number of edges, there a python loop with
 * two .item() read-backs per relation and layer).  Over the hop-`level` edges e = (b, h, rel, t) the forward aggregates (t in level
 * `level` of query b, h in level-1 of the same query; identity edges included, duplicated facts counted once each):
 *   count_out[b][rel] += number of such edges,   sum_out[b][rel] += sum of llrintf(alpha_e * 2^32)
 * with alpha_e of rg_layer_fwd, its arithmetic bit for bit (arguments as rg_explain_count: a_s of level-1 [n_old, ap], a_r
 * [n_rela_rows, ap], a_q [batch, ap], w_alpha, b_alpha).  sum_out / count_out: device int64 [batch][n_rela_rows], caller-owned and
 * caller-zeroed (or carrying earlier hops: the call adds).  alpha is summed as 64-bit fixed point with 32 fraction bits: the per-edge
 * rounding is q = 2^-33, the sum of a cell is exact in integers and therefore bit-identical across runs, across any split of the batch
 * and any order of its queries; alpha_sum = sum_out * 2^-32.  Needs a frontier that still holds levels level-1 and level with their
 * node counts known on the host (rg_frontier_expand); n_old is checked against it.  The relation bins live in LDS per workgroup (one
 * query per workgroup) and are flushed with non-returning 64-bit integer atomics.  The edges are enumerated from the heads (level
 * `level` is the set of tails of the out-edges of level-1, so these are all out-edges of the level-1 nodes: CSR by head, no candidate
 * read in vain); where n_rela_rows * (4 * ap + 12) bytes exceed 48 KB
 * the kernel adds per edge into sum_out / count_out directly (same result, slower).  attn_dim <= 32, batch <= 65535.  Allocates
 * nothing, asynchronous on `stream`. */
int rg_attn_profile(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                    const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha, const float* b_alpha,
                    int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream);

/* The attention profile of a hop of a temporal graph (T-RED-GNN interpolation), with the edge's direction as one more axis.  Edges,
 * enumeration, alpha (rg_tlayer_fwd's, which does not read the time; pass b_alpha = 0), fixed-point sums and limits are
 * rg_attn_profile's; per edge the kernel also reads the CSR-by-head entry's time id and bins by the forward's direction:
 * dt = edge time - q_time[b] (q_time device int32 [batch]), dir = 0 past (dt < 0), 1 now (dt == 0), 2 future (dt > 0):
 *   count_out[b][dir][rel] += 1,   sum_out[b][dir][rel] += llrintf(alpha_e * 2^32)
 * sum_out / count_out: device int64 [batch][3][n_rela_rows], caller-owned and caller-zeroed; a_r has n_rela_rows rows.  Summed over
 * dir this is the static table.  The bins live in LDS per workgroup where n_rela_rows * (4 * ap + 36) bytes fit 48 KB (722 relation
 * rows at ap = 8); above that the kernel adds per edge into the outputs directly (same integers, slower).  The graph must be temporal
 * and the frontier must have no window set (extrapolation is not supported). */
int rg_tattn_profile(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                     const int32_t* q_time, const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                     const float* b_alpha, int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream);

/* The attention profile of a hop of the extrapolation model (extrapolation.py's one-graph layout: the time field of an edge is its data
 * row, the frontier carries the queries' row windows), with the edge's lag in days, binned, as one more axis.  The edges are exactly the
 * hop-`level` edges rg_xlayer_fwd aggregates for query b: the out-edges of b's level-(level-1) nodes whose data row is a self-loop
 * (row >= n_data) or lies in [win_lo[b], win_hi[b]); n_data and the windows are the frontier's (rg_frontier_set_window), as for
 * rg_xexplain_*.  Enumeration, alpha (rg_xlayer_fwd's, which does not read the time; pass b_alpha = 0) and the fixed-point sums are
 * rg_attn_profile's.  Per edge the kernel forms the forward's time-table row
 *   lag = min(max(q_time[b] - (row >= n_data ? loop_time[b] : row_time[row]), 0), n_lag - 1),   bin = lag_bin[lag]
 * (q_time, loop_time device int32 [batch], row_time device int32 [n_data], lag_bin device uint8 [n_lag]) and adds
 *   count_out[b][bin][rel] += 1,   sum_out[b][bin][rel] += llrintf(alpha_e * 2^32)
 * sum_out / count_out: device int64 [batch][n_bins][n_rela_rows], caller-owned and caller-zeroed; the call adds.  An entry of lag_bin
 * >= n_bins drops the edge: whatever the table holds, nothing is written outside the outputs.  1 <= n_bins <= 256,
 * 1 <= n_lag <= 16384 (the table is staged in LDS).  Sums are exact integers: bit-identical across runs, across splits of a batch and
 * across query order.  The bins live in LDS per workgroup where
 *   16384 + n_rela_rows * (4 * ap + 12 * n_bins) + n_lag <= 81920 bytes (80 KiB: two workgroups per CU; 462 relation rows at ap = 8
 * with 8 bins fit) - which budget is faster has not been measured - and above that the kernel adds per edge into the outputs directly
 * (same integers, slower).  The graph must carry row ids (rg_tgraph_create) and the frontier must have its windows set.  Allocates
 * nothing, asynchronous on `stream`. */
int rg_xattn_profile(const rg_frontier* f, const rg_graph* g, int32_t batch, int32_t n_ent, int32_t level, int64_t n_old,
                     const int32_t* q_time, const int32_t* loop_time, const int32_t* row_time,
                     const uint8_t* lag_bin, int32_t n_lag, int32_t n_bins,
                     const float* a_s, const float* a_r, const float* a_q, int32_t ap, const float* w_alpha,
                     const float* b_alpha, int32_t attn_dim, int64_t* sum_out, int64_t* count_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* REDGNN_H */
