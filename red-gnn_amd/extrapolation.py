"""T_RED_GNN for temporal EXTRAPOLATION (forecasting) on the HIP path - inference and training.

Mirrors Temporal/extrapolation/model_cuda_new_embedding.py:57-265 (the reference's ``T_RED_GNN`` with the periodic time embedding):
parameters ``rela_embed_layer.{i}`` [n_rel + 2, d], ``attention_1_layer.{i}`` (3d -> a, no bias), ``attention_2_layer.{i}`` (a -> 1, no
bias), ``past_linear`` / ``now_linear`` / ``future_linear`` (only past_linear is used by the forward, :205), ``linear_classifier``,
``time_embed`` (+ the two absolute-time embeddings the reference constructs but does not use, :86-87).

What is different inside: the per-query python loop that slices ``self.dataset`` and stacks self-loops (:165-176), the scipy block
adjacency and the dense [B, n_ent] index maps (:178-191,229-235) and the pickled attention statistics (:145-152,216-220,254-259) do not
exist.  The whole data array lives on the device as ONE quadruple graph (self-loops first, then the time-sorted data rows, each edge
carrying its data-row index); a query's window ``dataset[time_offset_list[begin]:time_offset_list[cur_t]]`` is a pair of row bounds,
the frontier hops under those windows (rg_frontier_set_window) and the layer is one fused kernel (rg_xlayer_fwd) with the direction
matrix hoisted by linearity.  The time embedding of the ~120 distinct relative times of a window is a table computed once per forward.

Evaluation (main.py:353-472) stays on the device as well: ``known_objects_index`` stands in for the reference's sp2o / spt2o
dictionaries, ``T_RED_GNN.rank_batch`` ranks a batch's softmax scores raw, filtered and time-filtered in one HIP launch
(csrc/segment_rank.hip, rg_segment_rank) and ``T_RED_GNN.evaluate`` batches a split and returns the reference's metrics from one host
copy.  ``segment_rank_fil`` is the host restatement the device path is tested against.

Forecasts and their explanation: ``T_RED_GNN.predict(X, k, known)`` returns each query's k best objects among the entities its window
reaches, known objects excluded, in one HIP launch on the forward's pairs (csrc/segment_topk.hip, rg_segment_topk), and
``T_RED_GNN.explain(X, objs)`` the r-digraph of past facts behind a forecast, every edge with its attention and data row
(csrc/explain.hip, rg_xexplain_count / rg_xexplain_emit; the driver is explain.explain_extrapolation).  ``T_RED_GNN.attention_profile``
sums the attention of a batch's edges per hop, edge relation and lag bin (csrc/profile.hip, rg_xattn_profile; the driver is
profile.attention_profile_extrapolation), ``attention_profile_all`` over a split.  ``T_RED_GNN.rules`` / ``rules_all`` count the k
best paths behind forecasts as lag-binned rules (explain.LagRuleTable) and ``rule_quality`` counts how those hold in the model's own
data, per (entity, query day) anchor under the forward's row windows (csrc/xrule_ground.hip, rg_xrule_ground);
``rule_scores`` / ``rule_predict`` / ``rule_evaluate`` apply the weighted rules to queries (s, p, ?, t) under the same windows
(csrc/xrule_apply.hip, rg_xrule_apply; the drivers are explain.lag_rule_scores / lag_rule_predict / lag_rule_evaluate).
Explanation fidelity: ``rd.rescore(model, keep)`` re-scores a forecast on the kept edges of its r-digraph with the windows as they
were - per hop the index of the live edges built in HIP from the hop's own edges (csrc/digraph_index.hip, rg_digraph_hop_ranges /
rg_digraph_hop_index) and one rg_digraph_tlayer_fwd launch in its n_dir = 1 form; the driver is explain.rescore_extrapolation -,
``rd.fact_mask`` takes (s, p, o, day), ``rd.data_row_mask`` data rows, and ``T_RED_GNN.fidelity`` / ``fidelity_all`` measure what the
best k paths carry (explain.Fidelity).
Without gradients the per-row products of the forward (attention inputs, W_past products, time table, classifier) run through
rg_rows_linear (csrc/rows_linear.hip), whose rows do not depend on the row count: a query computes the same bits in every batch.

Parity: the reference's model file cannot be imported in the build container (torch_scatter, pyvis, rtdl_revisiting_models are absent),
so this path is checked against the oracle's restatement only - parity UNPINNED - except ``segment_rank_fil``, whose fixture comes
from the reference's importable ``segment.py``.
"""
import math
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import engine
from .models import pad_attn, tall_linear
from .profile import DEFAULT_LAG_EDGES


class _XAggregate(torch.autograd.Function):
    """agg = rg_xlayer_fwd(...);  backward = rg_xlayer_bwd(...).  The frontier keeps the batch's row windows until the backward has run
    (the lease holds it; T_RED_GNN.forward clears the windows only on the inference path)."""

    @staticmethod
    def forward(ctx, hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha, b_alpha, lease, graph, level, n_new, q_time, loop_time, row_time,
                n_data, d, attn_dim):
        hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha = (t.contiguous() for t in (hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha))
        agg = engine.xlayer_fwd(lease.frontier, graph, level, n_new, q_time, loop_time, row_time, n_data, hidden_p, rela_p, time_p, d,
                                a_s, a_r, a_q, w_alpha, b_alpha, attn_dim)
        ctx.save_for_backward(hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha, b_alpha, q_time, loop_time, row_time)
        ctx.misc = (lease, graph, level, n_data, d, attn_dim)
        return agg

    @staticmethod
    def backward(ctx, grad_agg):
        hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha, b_alpha, q_time, loop_time, row_time = ctx.saved_tensors
        lease, graph, level, n_data, d, attn_dim = ctx.misc
        lease.check()
        g = engine.xlayer_bwd(lease.frontier, graph, level, a_s.shape[0], q_time, loop_time, row_time, n_data, hidden_p, rela_p, time_p, d,
                              a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg)
        if level == 1:
            lease.release()
        return (g[0], g[1], g[2], g[3], g[4], g[5], g[6].view_as(w_alpha)) + (None,) * 11


WINDOW = 120        # model_cuda_new_embedding.py:168: begin_time = cur_t - 120


def _pad4(n):
    return (n + 3) // 4 * 4


def get_time_offset_list(data, time_granularity=24):
    """Temporal/extrapolation/utils.py:692-699, vectorised: offset_list[t + 1] = index of the LAST row whose time is t (0 where no row
    has that time - the reference's zeros stay)."""
    t = np.asarray(data)[:, 3] // time_granularity
    off = np.zeros(int(t.max()) + 2, dtype=np.int32)
    off[t + 1] = np.arange(len(t), dtype=np.int32)          # later rows overwrite earlier ones, as the reference's loop does
    return off


class PeriodicEmbeddings(nn.Module):
    """The reference's vendored (and edited) rtdl PeriodicEmbeddings for one feature, lite=False (rtdl_num_embeddings.py:69-100,126-215):
    x -> [cos(2 pi w x), sin(2 pi w x)] (n_frequencies each) -> one of two linears by the sign of x -> ReLU.  Same parameter names
    and shapes (``periodic.weight`` [1, k], ``linear_neg/linear_pos.weight`` [1, 2k, d], ``.bias`` [1, d]) and initialisation."""

    def __init__(self, d_embedding, n_frequencies=48, frequency_init_scale=0.01):
        super().__init__()
        self.periodic = nn.Module()
        self.periodic.weight = nn.Parameter(torch.empty(1, n_frequencies))
        nn.init.trunc_normal_(self.periodic.weight, 0.0, frequency_init_scale, a=-3 * frequency_init_scale, b=3 * frequency_init_scale)
        for name in ("linear_neg", "linear_pos"):
            lin = nn.Module()
            lin.weight = nn.Parameter(torch.empty(1, 2 * n_frequencies, d_embedding))
            lin.bias = nn.Parameter(torch.empty(1, d_embedding))
            r = (2 * n_frequencies) ** -0.5
            nn.init.uniform_(lin.weight, -r, r)
            nn.init.uniform_(lin.bias, -r, r)
            setattr(self, name, lin)

    def forward(self, x):
        """x [N, 1] -> [N, 1, d]."""
        is_neg = (x < 0).unsqueeze(-1)
        z = 2 * math.pi * self.periodic.weight * x[..., None]
        z = torch.cat([torch.cos(z), torch.sin(z)], -1)                                    # [N, 1, 2k]
        neg = (z[..., None, :] @ self.linear_neg.weight).squeeze(-2) + self.linear_neg.bias
        pos = (z[..., None, :] @ self.linear_pos.weight).squeeze(-2) + self.linear_pos.bias
        return torch.relu(neg * is_neg + pos * (~is_neg))


class T_RED_GNN(nn.Module):
    """``params``: n_ent, n_rel (true relations incl. reversed ones; the self-loop relation is id n_rel, as Data.num_relations),
    data int [n,4] = (subject, relation, object, time) sorted by time (contents.data), time_granularity, hidden_dim, attn_dim, n_layer,
    act, time_offset_list (optional: computed by get_time_offset_list)."""

    def __init__(self, params):
        super().__init__()
        self.n_rel_true = int(params.n_rel)
        self.n_rel = self.n_rel_true + 1                       # as the reference's self.n_rel (:61)
        self.n_ent, self.hidden_dim, self.attn_dim, self.n_layer = int(params.n_ent), params.hidden_dim, params.attn_dim, params.n_layer
        self.time_granularity = int(params.time_granularity)
        d, a = self.hidden_dim, self.attn_dim
        self.rela_embed_layer = nn.ModuleList([nn.Embedding(self.n_rel + 1, d) for _ in range(self.n_layer)])
        self.attention_1_layer = nn.ModuleList([nn.Linear(3 * d, a, bias=False) for _ in range(self.n_layer)])
        self.attention_2_layer = nn.ModuleList([nn.Linear(a, 1, bias=False) for _ in range(self.n_layer)])
        self.linear_classifier = nn.Linear(d, 1)
        self.past_linear = nn.Linear(d, d, bias=False)
        self.now_linear = nn.Linear(d, d, bias=False)
        self.future_linear = nn.Linear(d, d, bias=False)
        self.time_embed = PeriodicEmbeddings(d)
        self.time_embed_absolute_query = PeriodicEmbeddings(d)      # constructed, unused by the forward (:86-87,201)
        self.time_embed_absolute_graph = PeriodicEmbeddings(d)
        acts = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu, "idd": lambda x: x, "softplus": F.softplus,
                "leakyrelu": F.leaky_relu}
        self.act = acts[params.act]
        for i in range(self.n_layer):
            nn.init.xavier_normal_(self.rela_embed_layer[i].weight)   # init_params (:120-122)
        data = np.ascontiguousarray(np.asarray(params.data, dtype=np.int64).reshape(-1, 4))
        self.n_data = len(data)
        off = getattr(params, "time_offset_list", None)
        self.time_offset_list = np.asarray(off if off is not None else get_time_offset_list(data, self.time_granularity), dtype=np.int64)
        device = getattr(params, "device", "cuda")
        # one graph for every window: self-loops first (:172-173 puts them in front of a query's rows), then the data rows; the time
        # field of an edge is its data-row index (self-loops: n_data), which the kernels test against the query's row window
        ent = np.arange(self.n_ent)
        loops = np.stack([ent, np.full(self.n_ent, self.n_rel_true), ent, np.full(self.n_ent, self.n_data)], 1)
        rows = np.concatenate([data[:, :3], np.arange(self.n_data)[:, None]], 1)
        self.graph = engine.TemporalGraph(self.n_ent, self.n_rel + 1, self.n_data + 1, np.concatenate([loops, rows], 0).astype(np.int32),
                                          device=device)
        self._row_time_host = data[:, 3] // self.time_granularity
        self.register_buffer("row_time", torch.as_tensor(self._row_time_host, dtype=torch.int32), persistent=False)
        self._frontiers = engine.FrontierPool()
        self._anchors = None                                   # default_anchors(), formed on first use
        self.last_stats = None

    def forward(self, X):
        """X: src_idx, rel_idx, ts (numpy arrays, as the reference's batch object).  Returns (score_all [B, n_ent],
        (per-query softmax over the visited entities [N], visited (batch, entity) pairs int64 numpy [N,2])) as :245-261."""
        _, soft, nodes, score_all = self._run(X, dense=True)
        return score_all, (soft, nodes.long().cpu().numpy())

    def _run(self, X, dense=False, kept=None):
        """The forward on the device: (logits [N], per-query softmax [N], visited (batch, entity) pairs int32 [N,2] sorted, score_all) -
        score_all [B, n_ent] only with ``dense`` (else None: nothing of size B * n_ent is built, nothing is copied to the host).
        ``kept`` (a list, for explain): the frontier keeps all n_layer + 1 levels and its windows stay set - the caller clears them; the
        list receives dict(frontier, graph, q_rel, q_time, loop_time, win_lo, win_hi, n_tab = the rows of the forward's time table),
        then per layer dict(a_s, a_r, a_q, w_alpha)."""
        device = self.linear_classifier.weight.device
        engine._require_gpu(device)
        src, rel = np.asarray(X.src_idx), np.asarray(X.rel_idx)
        cur_t = np.asarray(X.ts) // self.time_granularity                          # :138
        n = len(src)
        begin = np.maximum(cur_t - WINDOW, 0)                                       # :168-170
        off = self.time_offset_list
        to32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(device)
        win_lo, win_hi = to32(off[begin]), to32(off[cur_t])                         # :171 dataset[offset[begin]:offset[cur_t]]
        q_time, loop_time = to32(cur_t), to32(begin)                                # self-loops carry time begin * granularity (:172)
        q_rel = torch.as_tensor(rel, dtype=torch.int64).to(device)
        with_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        fr = self._frontiers.get(self.n_ent, n, self.n_layer + 1 if with_grad or kept is not None else 2, device)
        fr.set_window(win_lo, win_hi, self.n_data)
        if kept is not None:
            kept.append(dict(frontier=fr, graph=self.graph, q_rel=q_rel, q_time=q_time, loop_time=loop_time, win_lo=win_lo, win_hi=win_hi))
        fr.reset(to32(src))
        lease = engine.FrontierLease(fr) if with_grad else None
        d, a = self.hidden_dim, self.attn_dim
        ld, ap = max(16, _pad4(d)), pad_attn(a)
        padc = lambda t: F.pad(t, (0, ld - d)) if ld != d else t
        pad_rows = lambda w: F.pad(w, (0, 0, 0, ap - a)) if ap != a else w
        w_past = self.past_linear.weight
        # largest relative time any edge of the batch can have: a window's oldest row is its first (the data are time-sorted; the
        # reference's offsets put the last row of the day before `begin` in front, and 0 for days without rows)
        lo_h, hi_h = off[begin], off[cur_t]
        oldest = np.where(lo_h < hi_h, self._row_time_host[np.minimum(lo_h, self.n_data - 1)], begin) if self.n_data else begin
        n_tab = int(np.maximum(cur_t - oldest, cur_t - begin).max()) + 1 if n else 1
        if kept is not None:
            kept[0]["n_tab"] = n_tab
        deltas = torch.arange(n_tab, dtype=torch.float32, device=device)
        hidden = torch.zeros((n, d), device=device)
        zero_b = torch.zeros(1, device=device)
        n_edges = []
        with torch.set_grad_enabled(with_grad):
            # the per-row products: autograd's library GEMMs when training; without gradients rg_rows_linear, whose rows do not depend
            # on the row count, so that a query computes the same bits in every batch (the library picks its kernel by the shape)
            lin = tall_linear if with_grad else engine.rows_linear
            if with_grad:
                t_emb = self.time_embed(deltas.view(-1, 1)).squeeze(1)
            else:                                    # time_embed for x >= 0: relu(linear_pos([cos | sin](2 pi w x))) (PeriodicEmbeddings.forward)
                z = 2 * math.pi * self.time_embed.periodic.weight * deltas.view(-1, 1)
                pos = self.time_embed.linear_pos
                t_emb = torch.relu(lin(torch.cat([torch.cos(z), torch.sin(z)], -1), pos.weight[0].t(), pos.bias[0]))
            time_p = padc(lin(t_emb, w_past)).contiguous()                                                   # W_past time_embed(delta)  (:201,205)
            for i in range(self.n_layer):
                rela, w1, w2 = self.rela_embed_layer[i].weight, self.attention_1_layer[i].weight, self.attention_2_layer[i].weight
                n_new, n_e, n_old = fr.expand(self.graph)
                n_edges.append(n_e)
                a_s = lin(hidden, pad_rows(w1[:, :d])).contiguous()                       # attention_1 on [h_s | rel | rel_q] (:207-208)
                a_r = F.linear(rela, pad_rows(w1[:, d:2 * d])).contiguous()
                a_q = lin(rela[q_rel], pad_rows(w1[:, 2 * d:])).contiguous()
                hidden_p = padc(lin(hidden, w_past)).contiguous()                         # W_past (h + r + tau) = W_past h + ... (:203-205)
                rela_p = padc(F.linear(rela, w_past)).contiguous()
                w_alpha = w2.reshape(-1).contiguous()
                if kept is not None:
                    kept.append(dict(a_s=a_s, a_r=a_r, a_q=a_q, w_alpha=w_alpha))
                if with_grad:
                    agg = _XAggregate.apply(hidden_p, rela_p, time_p, a_s, a_r, a_q, w_alpha, zero_b, lease, self.graph, fr.level, n_new,
                                            q_time, loop_time, self.row_time, self.n_data, d, a)
                else:
                    agg = engine.xlayer_fwd(fr, self.graph, fr.level, n_new, q_time, loop_time, self.row_time, self.n_data, hidden_p, rela_p,
                                            time_p, d, a_s, a_r, a_q, w_alpha, zero_b, a)
                hidden = self.act(agg[:, :d])                                                     # :238-239
            nodes, _, _ = fr.nodes(want_prev=False, want_old_new=False)
            result = lin(hidden, self.linear_classifier.weight, self.linear_classifier.bias).reshape(-1)   # :244
            b_idx = nodes[:, 0].long()
            score_all = None
            if dense:
                score_all = torch.zeros(n * self.n_ent, device=device).index_copy(0, b_idx * self.n_ent + nodes[:, 1].long(), result)
                score_all = score_all.view(n, self.n_ent)
            # scatter_softmax(result, cur_entity[:, 0]) (:248): per-query softmax over the visited entities
            row_max = torch.full((n,), float("-inf"), device=device).scatter_reduce(0, b_idx, result.detach(), "amax")
            ex = torch.exp(result - row_max[b_idx])
            soft = ex / torch.zeros(n, device=device).index_add(0, b_idx, ex)[b_idx]
        if not with_grad and kept is None:
            fr.set_window(None, None, 0)         # (a training forward's frontier keeps its windows for the backward: every reset sets them anew)
        self.last_stats = dict(n_edges=n_edges, n_nodes=int(nodes.shape[0]), n_tab=n_tab)
        return result, soft, nodes, score_all

    def _index_on_device(self, index, device):
        """A KnownObjects index as device tensors, copied once per index and device and kept on the model (the last few)."""
        cache = self.__dict__.setdefault("_known_dev", {})
        key = (id(index), str(device))
        hit = cache.get(key)
        if hit is None or hit[0] is not index:
            while len(cache) >= 8:
                cache.pop(next(iter(cache)))
            hit = cache[key] = (index, _index_tensors(index, device))
        return hit[1]

    def rank_batch(self, X, targets, sp_index=None, spt_index=None):
        """Ranks of one batch as main.py:383,404 computes them, on the device: the forward, then the rank of every query's target among
        ITS visited entities by the per-query softmax - raw, filtered by the other known objects of (s, p) (``sp_index``) and of
        (s, p, ts) (``spt_index``), both from known_objects_index; None filters nothing.  X as forward's; ``targets`` int [B].
        Runs without gradients in eval mode (the training flags come back).  Returns a RankBatch of device tensors."""
        from .temporal import eval_semantics
        device = engine._require_gpu(self.linear_classifier.weight.device)
        src, rel, ts = (_int_ids(x, "rank_batch", k) for x, k in ((X.src_idx, "src_idx"), (X.rel_idx, "rel_idx"), (X.ts, "ts")))
        tgt = _int_ids(targets, "rank_batch", "targets")
        n = len(src)
        if n == 0 or len(rel) != n or len(ts) != n or len(tgt) != n:
            raise ValueError("rank_batch: need one relation, time and target per subject and at least one query (got %d, %d, %d, %d)"
                             % (n, len(rel), len(ts), len(tgt)))
        with torch.no_grad(), eval_semantics(self):
            _, soft, nodes, _ = self._run(X, dense=False)
            # nodes are sorted by (query, entity): query q owns the pairs seg_ptr[q]:seg_ptr[q+1]
            seg_ptr = torch.searchsorted(nodes[:, 0].contiguous(), torch.arange(n + 1, dtype=torch.int32, device=device))
            ent = nodes[:, 1].contiguous()
            keys, known = [], []
            for index in (sp_index, spt_index):
                keys.append(None if index is None else torch.as_tensor(index.query_keys(src, rel, ts)).to(device))
                known.append(None if index is None else self._index_on_device(index, device))
            rank, rank_fil, rank_fil_t, found = engine.segment_rank(soft.contiguous(), ent, seg_ptr, torch.as_tensor(tgt, dtype=torch.int32).to(device),
                                                                    keys[0], known[0], keys[1], known[1])
        return RankBatch(rank=rank, found=found.bool(), rank_fil=rank_fil, rank_fil_t=rank_fil_t, soft=soft, nodes=nodes)

    def predict(self, X, k=10, known=None):
        """The k best forecasts of every query (s, p, ?, t) among the entities its window reaches - the reference ranks a query only
        there (main.py:383) - without those ``known`` lists for it: a KnownObjects index of the (s, p) or the (s, p, t) kind
        (known_objects_index); None excludes nothing.  X as forward's.  Returns prediction.Prediction: ids int64 [B, k] (-1 where the
        query has fewer than k candidates), scores = the logits (-inf there), prob = the per-query softmax over ALL visited entities
        (0 there), ordered by logit descending, then entity id ascending.  The forward without the [B, n_ent] matrix, then one HIP
        launch (csrc/segment_topk.hip); nothing is copied to the host.  No gradients, eval mode (the training flags come back)."""
        from .prediction import K_MAX, Prediction
        from .temporal import eval_semantics
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
            raise ValueError("predict: k must be an integer in 1..%d (got %r)" % (K_MAX, k))
        k = int(k)
        if not 1 <= k <= K_MAX:
            raise ValueError("predict: k=%d not in 1..%d" % (k, K_MAX))
        src, rel, ts = check_batch(self, X, "predict")
        device = engine._require_gpu(self.linear_classifier.weight.device)
        n = len(src)
        with torch.no_grad(), eval_semantics(self):
            logits, _, nodes, _ = self._run(X, dense=False)
            seg_ptr = torch.searchsorted(nodes[:, 0].contiguous(), torch.arange(n + 1, dtype=torch.int32, device=device))
            q_key = known_dev = None
            if known is not None:
                q_key = torch.as_tensor(known.query_keys(src, rel, ts)).to(device)
                known_dev = self._index_on_device(known, device)
            idx, val, prob = engine.segment_topk(logits.contiguous(), nodes[:, 1].contiguous(), seg_ptr, k, q_key, known_dev)
        return Prediction(ids=idx.long(), scores=val, prob=prob)

    def explain(self, X, objs=None, min_alpha=0.0):
        """The past facts a forecast is built on: for row b = (s, p, t) of X and the answer objs[b] (None: the row's own top
        forecast, predict(k=1) without a filter) the r-digraph of explain.RDigraph - the union of the length-L paths s -> o inside the
        row's window, every edge with its attention alpha (>= min_alpha; the paths are re-closed after the cut).  ``data_row`` is the
        edge's index into the model's data array (-1 for a self-loop, whose relation id is n_rel), ``time`` the day the forward used
        for it, ``q_time`` the query's day and ``lag()`` their difference.  Extraction in HIP (rg_xexplain_*, csrc/explain.hip)."""
        from .explain import explain_extrapolation
        return explain_extrapolation(self, X, objs, min_alpha)

    def attention_profile(self, X, group="relation", lag_edges=DEFAULT_LAG_EDGES):
        """When the model forecasts relation p, which past relations does it listen to, and how far back?  profile.AttentionProfile
        with axes ("group", "hop", "lag", "relation"), shape [G, L, len(lag_edges) + 1, n_rel + 1]: over the hop-l edges the forward
        aggregates for the queries of X (as forward's), the number of edges and the sum of their attention per edge relation and lag
        bin - the edge's lag in days (query day minus the edge's day) binned by ``lag_edges`` (profile.DEFAULT_LAG_EDGES: days 0-1,
        2-3, 4-7, 8-14, 15-30, 31-60, 61-120, 121+; lags above 120 occur: the reference's offsets put older rows in front of a window
        after days without rows).  G = the n_rel + 1 relation rows (group="relation", rows of relations not queried are zero) or the B
        queries in the order given (group="query").  The self-loop of every visited entity is an edge too: it lands in the self-loop
        relation's column, n_rel_true, at the lag the forward uses for it (query day minus the window's first day, 120 for a full
        window) - leave that column out to see data rows only.  One forward, then one HIP launch per hop (rg_xattn_profile,
        csrc/profile.hip); integer sums, bit-identical across runs, splits and orders of a batch.  No gradients, eval mode."""
        from .profile import attention_profile_extrapolation
        return attention_profile_extrapolation(self, X, group, lag_edges)

    def attention_profile_all(self, queries, batch_size=64, lag_edges=DEFAULT_LAG_EDGES):
        """The group="relation" attention profile of ``queries`` int [n, 4] = (s, p, o, ts) (checked as evaluate's; the objects are
        not read), in batches of ``batch_size``, their integer tables added."""
        q = check_queries(self, queries, batch_size, "attention_profile_all")
        prof = None
        for lo in range(0, len(q), int(batch_size)):
            b = q[lo:lo + int(batch_size)]
            part = self.attention_profile(_Batch(b[:, 0], b[:, 1], b[:, 3]), "relation", lag_edges)
            prof = part if prof is None else prof + part
        return prof

    def rules(self, X, objs=None, k=1, lag_edges=DEFAULT_LAG_EDGES, min_alpha=0.0):
        """The k best paths behind the forecast of every row of X (as forward's) counted as lag-binned rules: explain -> top_paths(k)
        -> explain.LagRuleTable, one row per distinct (query relation, (relation, lag bin) of every step).  The lag of a step is the
        query day minus the day of its fact, binned by ``lag_edges`` as attention_profile bins it; identity steps are written as
        ANY.  objs=None: each row's own top forecast, as explain."""
        from . import explain as _explain
        edges = _explain.check_lag_edges(lag_edges)
        rd = self.explain(X, objs, min_alpha)
        return _explain.lag_rules_from_paths(rd.top_paths(k), np.asarray(X.rel_idx), self.n_rel_true, edges)

    def rules_all(self, queries, k=1, batch_size=64, lag_edges=DEFAULT_LAG_EDGES):
        """The rule tables of ``queries`` int [n, 4] = (s, p, o, ts) (checked as evaluate's) - each row a query with its object as
        the answer - walked in batches of ``batch_size`` rows and added (tables add exactly)."""
        q = check_queries(self, queries, batch_size, "rules_all")
        table = None
        for lo in range(0, len(q), int(batch_size)):
            b = q[lo:lo + int(batch_size)]
            t = self.rules(_Batch(b[:, 0], b[:, 1], b[:, 3]), b[:, 2], k=k, lag_edges=lag_edges)
            table = t if table is None else table + t
        return table

    def fidelity(self, X, objs=None, k=4, inverse_offset=None):
        """How much of a forecast its best paths carry: for every row of X (as forward's) and the answer objs[b] (None: the row's own
        top forecast, as rules) an explain.Fidelity - explain -> top_paths(k), then for j = 1..k the answer re-scored without the
        past facts of the best j paths (``without``) and with only them and the self-loops (``only``), by RDigraph.rescore on the
        digraph's own edge list (rg_digraph_hop_index, rg_digraph_tlayer_fwd).  A fact is (s, p, o, day) and is deleted for its own
        row at every hop, every copy of it; with ``inverse_offset`` = m its twin (o, p + m or p - m, s, day) goes too - how a
        dataset writes reversed relations belongs to the data.  The windows stay as they were (RDigraph.rescore).  No gradients,
        eval mode (the training flags come back)."""
        from .explain import extrapolation_fidelity
        return extrapolation_fidelity(self, X, objs, k, inverse_offset)

    def saliency(self, X, objs=None):
        """How much a forecast depends on every past fact of its r-digraph, in one pass: ``explain`` followed by RDigraph.saliency -
        the gradient of the score with respect to a gate on every edge's message, the windows as they were (the timed edge-list
        layer's adjoint in HIP, rg_digraph_tlayer_bwd in its n_dir = 1 form).  Returns an explain.Saliency: ``edge_grad`` per edge of
        ``.digraph``, ``fact_grad()`` / ``top(k)`` per fact (s, p, o, day), ``data_row_grad()`` per data row, ``deletion_estimate(mask)``
        the first-order estimate of a rescore.  objs=None: the row's own top forecast, as explain.  Eval semantics; the parameters
        get no gradient."""
        return self.explain(X, objs).saliency(self)

    def fidelity_all(self, queries, k=4, batch_size=64, inverse_offset=None):
        """fidelity over ``queries`` int [n, 4] = (s, p, o, ts) (checked as evaluate's), each row a query with its object as the
        answer, in batches of ``batch_size``: the dict of BaseModel.fidelity - n, k, necessity_mean / _median, sufficiency_gap_mean /
        _median and disconnected (the share of reached answers the deletion cuts off), a list over j = 1..k each."""
        from .explain import extrapolation_fidelity_all
        return extrapolation_fidelity_all(self, queries, k, batch_size, inverse_offset)

    def windows(self):
        """(win_lo, win_hi) int64 [n_day]: the forward's row window [off[max(t - 120, 0)], off[t]) of every query day t, off being
        time_offset_list (as _run forms it per query)."""
        off = self.time_offset_list
        t = np.arange(len(off))
        return off[np.maximum(t - WINDOW, 0)], off[t]

    def default_anchors(self):
        """int64 [S, 2] = (entity, day) sorted by (day, entity): the distinct (subject, day) pairs of the data rows."""
        if self._anchors is None:
            self._anchors = engine.xrule_default_anchors(self.graph, self._row_time_host)
        return self._anchors

    def rule_quality(self, table, anchors=None, scratch_bytes=engine.RULE_SCRATCH_BYTES):
        """How the rules of ``table`` (an explain.LagRuleTable) hold in the model's own data: explain.LagRuleQuality with the exact
        counts body_pairs, hits, pca_body_pairs and head_pairs of every rule over the pairs ((x, t), y), (x, t) an anchor -
        ``anchors`` int [S, 2] = (entity, query day), distinct; None: every (subject, day) of the data rows - counted in HIP
        (rg_xrule_ground), independent of ``scratch_bytes``, which bounds the bitmaps of a chunk.

        body_pairs: the (anchor, y) pairs the body connects through rows of day t's window - the forward's, with the reference's
        offsets as they are - whose lag lies in each step's bin.  hits: those with a row (x, head, y) on day t itself.
        pca_body_pairs: the body's pairs whose anchor has some head fact on day t.  head_pairs: the head facts of the anchors' days.
        The counts are taken on the model's own data, so ``hits`` says how often a rule reproduces known facts of the query day, not
        held-out ones.  No window holds a row of the query day, so no rule is trivial."""
        from . import explain as _explain
        if not isinstance(table, _explain.LagRuleTable):
            raise ValueError("rule_quality: table must be an explain.LagRuleTable (got %s)" % type(table).__name__)
        if table.n_rel != self.n_rel_true:
            raise ValueError("rule_quality: the table has n_rel=%d, the model n_rel=%d" % (table.n_rel, self.n_rel_true))
        if anchors is None:
            anchors = self.default_anchors()
        lag_lo, lag_hi = table.lag_ranges()
        win_lo, win_hi = self.windows()
        counts = engine.xrule_ground(self.graph, table.head, table.body, lag_lo, lag_hi, self._row_time_host, win_lo, win_hi, anchors,
                                     WINDOW, scratch_bytes)
        return _explain.LagRuleQuality(table, *(counts[:, c].contiguous() for c in range(4)), int(len(anchors)))

    def rule_scores(self, quality, X, by="confidence", laplace=0.0, min_hits=1, scratch_bytes=engine.RULE_SCRATCH_BYTES):
        """What the rules of ``quality`` (an explain.LagRuleQuality, from rule_quality) forecast for the queries (s, p, ?, t) of X (as
        forward's; day = ts // time_granularity; a batch without rows is allowed) on the model's own data, in HIP (rg_xrule_apply):
        explain.RuleScores with best / surv / best_rule / fired [B, n_ent].  A rule fires for (b, y) iff its head is the query
        relation and its steps lead from the subject to y through rows of the query day's window - the forward's, windows() - whose
        lag lies in each step's bin, exactly as rule_quality counts a body for an anchor of that day; a self-loop has the lag
        min(day, 120).  The rules kept and their weights are explain.rule_weights(quality, by, laplace, min_hits); ``best_rule`` holds
        table rows.  No bit depends on ``scratch_bytes``, which bounds the bitmaps of one call."""
        from . import explain as _explain
        return _explain.lag_rule_scores(self, quality, X, by, laplace, min_hits, scratch_bytes)

    def rule_predict(self, quality, X, k=10, agg="noisy_or", known=None, **weights):
        """The k best forecasts of every query of X by rule score alone (agg "noisy_or": 1 - the product of the firing rules'
        1 - weight; "max": the largest weight), selected in HIP (rg_topk) over all entities: explain.RulePrediction, score descending
        then entity id ascending, -1 / -inf / -1 / 0 past the end, ``rule`` the table row of each answer's best rule and ``table`` the
        LagRuleTable, so format() prints the rule with its lag tags.  ``known``: a KnownObjects index of the (s, p) or the (s, p, t)
        kind (known_objects_index); the objects it lists for a query are left out.  ``weights``: by, laplace, min_hits, scratch_bytes
        of rule_scores.  A batch without rows gives [0, k] tensors."""
        from . import explain as _explain
        return _explain.lag_rule_predict(self, quality, X, k, agg, known, **weights)

    def rule_evaluate(self, queries, quality=None, mine=None, k=1, agg="noisy_or", sp_index=None, spt_index=None, batch_size=256,
                      lag_edges=DEFAULT_LAG_EDGES, anchors=None, **weights):
        """Ranking metrics of the rules alone on ``queries`` int [n, 4] = (s, p, o, ts) (checked as evaluate's), next to evaluate:
        exactly one of ``quality`` (a LagRuleQuality) and ``mine`` (int [m, 4] queries: rules_all(mine, k, lag_edges=lag_edges) ->
        rule_quality(table, anchors)) is given.  Per batch of ``batch_size`` queries the rule scores (rule_scores, ``agg``) are ranked
        over all n_ent entities by rg_rank three times - raw, filtered by the other known objects of (s, p) (``sp_index``) and of
        (s, p, ts) (``spt_index``), both from known_objects_index; a query's filter set is its object and the objects the index
        lists for it.  Returns a dict: n, coverage (the share of objects some rule reaches) and hits1 / hits3 / hits10 / mrr / mr with
        the suffixes "" / _fil / _fil_t, sums in float64.  ``weights``: by, laplace, min_hits, scratch_bytes of rule_scores.

        When it mines (``mine``) and ``anchors`` is None, the confidences are counted on the default anchors whose day is BELOW THE
        EARLIEST QUERY DAY, not on all of them: the model's data may hold the evaluated rows themselves, and a rule must not be
        weighted by the facts it is then scored on.  ValueError if that leaves no anchor.  Given anchors are used as they are.

        Two differences from evaluate: the ranks are over every entity, not over the ones the query's window reaches, and rg_rank's
        tie term counts every entity that scores exactly as the object, filtered ones included (the convention of
        BaseModel.rule_evaluate): every entity no rule reaches scores 0."""
        from . import explain as _explain
        return _explain.lag_rule_evaluate(self, queries, quality, mine, k, agg, sp_index, spt_index, batch_size, lag_edges, anchors,
                                          **weights)

    def evaluate(self, queries, sp_index=None, spt_index=None, batch_size=64, return_ranks=False):
        """The validation loop of main.py:353-472 for a split: ``queries`` int [n, 4] = (s, p, o, ts), in batches of ``batch_size``
        through rank_batch; the rank tensors stay on the device and are copied to the host once.  Returns the reference's quantities
        with its denominators: hits1 / hits3 / hits10 / mrr (raw, :413-415,426), *_fil (:416-418,429) and *_fil_t (:419-421,430; the
        reference's time-filtered list holds found queries only) over the number of queries, hits_inf = found / n, mr (:423), and
        among the found queries hits1_found / hits3_found / hits10_found / mr_found / mrr_found (:455-462; NaN when none is found).
        Sums in float64.  ``return_ranks``: also (rank, found, rank_fil, rank_fil_t) as numpy arrays [n] (unfound: 1e9)."""
        q = check_queries(self, queries, batch_size, "evaluate")
        parts = []
        for lo in range(0, len(q), int(batch_size)):
            b = q[lo:lo + int(batch_size)]
            r = self.rank_batch(_Batch(b[:, 0], b[:, 1], b[:, 3]), b[:, 2], sp_index, spt_index)
            parts.append(torch.stack([r.rank, r.found.float(), r.rank_fil, r.rank_fil_t]))
        rank, found, rank_fil, rank_fil_t = torch.cat(parts, 1).cpu().numpy().astype(np.float64)      # the one host copy
        found = found != 0
        out = extrapolation_metrics(rank, found, rank_fil, rank_fil_t[found])
        return (out, (rank, found, rank_fil, rank_fil_t)) if return_ranks else out


def segment_rank_fil(t, entities, target_idx_l, sp2o, spt2o, queries_sub, queries_pre, queries_ts):
    """Temporal/extrapolation/segment.py:346-387 with the same arguments and results (rank, found_mask, rank_fil, rank_fil_t): the
    rank of every query's target among ITS visited entities by score ``t`` (ties count half), raw, filtered by the other known
    objects of (s, p) and by those of (s, p, ts).  numpy per segment instead of a Python list comprehension per entity."""
    t = np.asarray(t.detach().cpu() if torch.is_tensor(t) else t)
    entities = np.asarray(entities)
    mask = entities[1:, 0] != entities[:-1, 0]
    key_idx = np.concatenate([[0], np.arange(1, len(entities))[mask], [len(entities)]]).astype(np.int64)
    rank, rank_fil, rank_fil_t, found = [], [], [], []
    for i, (s, e) in enumerate(zip(key_idx[:-1], key_idx[1:])):
        ents, sc = entities[s:e, 1], t[s:e]
        arg = np.nonzero(ents == target_idx_l[i])[0]
        if arg.size == 0:
            found.append(False); rank.append(1e9); rank_fil.append(1e9)        # (rank_fil_t gets no entry: as the reference)
            continue
        found.append(True)
        ts = sc[arg]

        def one(keep):
            return float(np.sum(sc[keep] > ts)) + (float(np.sum(sc[keep] == ts)) - 1) / 2 + 1

        everything = np.ones(len(ents), dtype=bool)
        rank.append(one(everything))
        other = np.setdiff1d(sp2o[(queries_sub[i], queries_pre[i])], [target_idx_l[i]])
        rank_fil.append(one(~np.isin(ents, other)))
        other_t = np.setdiff1d(spt2o[(queries_sub[i], queries_pre[i], queries_ts[i])], [target_idx_l[i]])
        rank_fil_t.append(one(~np.isin(ents, other_t)))
    return np.array(rank), found, np.array(rank_fil), np.array(rank_fil_t)


class _Batch:
    """The fields of the reference's batch object that the forward reads."""
    __slots__ = ("src_idx", "rel_idx", "ts")

    def __init__(self, src_idx, rel_idx, ts):
        self.src_idx, self.rel_idx, self.ts = src_idx, rel_idx, ts


@dataclass
class RankBatch:
    """T_RED_GNN.rank_batch: rank, rank_fil, rank_fil_t float32 [B] (1e9 where the target was not reached), found bool [B], soft
    float32 [N] (the per-query softmax that was ranked) and nodes int32 [N, 2] (its (query, entity) pairs), on the model's device."""
    rank: torch.Tensor
    found: torch.Tensor
    rank_fil: torch.Tensor
    rank_fil_t: torch.Tensor
    soft: torch.Tensor
    nodes: torch.Tensor


class KnownObjects(tuple):
    """(keys int64 sorted and unique, ptr int64 [len(keys) + 1], idx int32): the objects of key i are idx[ptr[i]:ptr[i+1]], ascending and
    unique - the layout of prediction.temporal_known_index.  key = s * n_rel_rows + p, and with ``n_time`` > 0
    (s * n_rel_rows + p) * n_time + t for the raw timestamp t.  Unpacks as the three arrays."""

    def __new__(cls, keys, ptr, idx, n_rel_rows, n_time=0):
        self = super().__new__(cls, (np.ascontiguousarray(keys, dtype=np.int64), np.ascontiguousarray(ptr, dtype=np.int64),
                                     np.ascontiguousarray(idx, dtype=np.int32)))
        self.n_rel_rows, self.n_time = int(n_rel_rows), int(n_time)
        return self

    def query_keys(self, s, p, t=None):
        """int64 keys of the queries (s, p[, t]); -1, which no index holds, where p or t lies outside the index's ranges."""
        s, p = np.asarray(s, dtype=np.int64), np.asarray(p, dtype=np.int64)
        ok = (s >= 0) & (p >= 0) & (p < self.n_rel_rows)
        key = s * self.n_rel_rows + p
        if self.n_time:
            t = np.asarray(t, dtype=np.int64)
            ok &= (t >= 0) & (t < self.n_time)
            key = key * self.n_time + t
        return np.where(ok, key, -1).astype(np.int64)

    def objects(self, s, p, t=None):
        """The objects of one key, as the reference's dictionary lookup (empty when absent)."""
        k = int(self.query_keys([s], [p], None if t is None else [t])[0])
        i = int(np.searchsorted(self[0], k))
        if i == len(self[0]) or self[0][i] != k:
            return np.zeros(0, np.int32)
        return self[2][self[1][i]:self[1][i + 1]]


def known_objects_index(quads, n_rel_rows, with_time):
    """The known objects of (s, p) - the reference's get_sp2o() over all data (utils.py:228-240) - or, ``with_time``, of (s, p, t) -
    get_spt2o(split) over one split (:207-226) - from quadruples int [n, 4] = (s, p, o, raw timestamp), as a KnownObjects index.
    Vectorised as prediction.temporal_known_index: one np.unique over (key, object) pairs.  With time, n_time = max timestamp + 1."""
    q = np.asarray(quads)
    if q.size and (q.dtype == np.bool_ or not np.issubdtype(q.dtype, np.integer)):
        raise ValueError("known_objects_index: quads must hold integer ids (got dtype %s)" % q.dtype)
    q = q.astype(np.int64).reshape(-1, 4)
    if len(q) and (q.min() < 0 or q[:, 1].max() >= n_rel_rows):
        raise ValueError("known_objects_index: negative id or relation id out of range (n_rel_rows=%d)" % n_rel_rows)
    n_time = (int(q[:, 3].max()) + 1 if len(q) else 1) if with_time else 0
    key = q[:, 0] * n_rel_rows + q[:, 1]
    if with_time:
        key = key * n_time + q[:, 3]
    pairs = np.unique(np.stack([key, q[:, 2]], 1), axis=0) if len(q) else np.zeros((0, 2), np.int64)      # sorted by (key, object)
    keys, first = np.unique(pairs[:, 0], return_index=True)
    return KnownObjects(keys, np.append(first, len(pairs)), pairs[:, 1], n_rel_rows, n_time)


def _int_ids(x, who, name):
    a = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).reshape(-1)
    if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):      # (no silent truncation of 1.7 to 1)
        raise ValueError("%s: %s must hold integer ids (got dtype %s)" % (who, name, a.dtype))
    return a.astype(np.int64)


def check_batch(model, X, who):
    """(src, rel, ts) int64 [B] of a batch object, checked on the host as evaluate checks its queries: integer ids, one relation and
    time per subject, at least one query, ids and times inside the model's data."""
    src, rel, ts = (_int_ids(x, who, k) for x, k in ((X.src_idx, "src_idx"), (X.rel_idx, "rel_idx"), (X.ts, "ts")))
    n = len(src)
    if n == 0 or len(rel) != n or len(ts) != n:
        raise ValueError("%s: need one relation and time per subject and at least one query (got %d, %d, %d)" % (who, n, len(rel), len(ts)))
    if src.min() < 0 or src.max() >= model.n_ent or rel.min() < 0 or rel.max() >= model.n_rel_true:
        raise ValueError("%s: subject / relation id out of range (n_ent=%d, n_rel=%d)" % (who, model.n_ent, model.n_rel_true))
    if ts.min() < 0 or (ts // model.time_granularity).max() >= len(model.time_offset_list):
        raise ValueError("%s: query time outside the model's data (0 <= ts // %d < %d)"
                         % (who, model.time_granularity, len(model.time_offset_list)))
    return src, rel, ts


def check_queries(model, queries, batch_size, who):
    """``queries`` as int64 [n, 4] = (s, p, o, ts) with ids and times inside the model's data; ValueError otherwise."""
    q = queries.detach().cpu().numpy() if torch.is_tensor(queries) else np.asarray(queries)
    if q.dtype == np.bool_ or not np.issubdtype(q.dtype, np.integer):
        raise ValueError("%s: queries must hold integer ids (got dtype %s)" % (who, q.dtype))
    if q.ndim != 2 or q.shape[1] != 4 or len(q) == 0:
        raise ValueError("%s: queries must be a non-empty int [n, 4] array of (s, p, o, ts) (got shape %s)" % (who, q.shape))
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError("%s: batch_size must be a positive integer (got %r)" % (who, batch_size))
    q = q.astype(np.int64)
    if q[:, [0, 2]].min() < 0 or q[:, [0, 2]].max() >= model.n_ent or q[:, 1].min() < 0 or q[:, 1].max() >= model.n_rel_true:
        raise ValueError("%s: subject / object / relation id out of range (n_ent=%d, n_rel=%d)" % (who, model.n_ent, model.n_rel_true))
    day = q[:, 3] // model.time_granularity
    if q[:, 3].min() < 0 or day.max() >= len(model.time_offset_list):
        raise ValueError("%s: query time outside the model's data (0 <= ts // %d < %d)"
                         % (who, model.time_granularity, len(model.time_offset_list)))
    return q


def _index_tensors(index, device):
    return tuple(torch.as_tensor(a).to(device).contiguous() for a in index)


def segment_rank_fil_device(t, entities, target_idx_l, sp_index, spt_index, queries_sub, queries_pre, queries_ts, device="cuda"):
    """segment_rank_fil computed by rg_segment_rank: the same arguments with KnownObjects indexes (known_objects_index) in place of the
    two dictionaries, the same results (rank [B], found list, rank_fil [B], rank_fil_t compacted to the found queries).  ``t`` and
    ``entities`` may be device tensors; the segments are the runs of entities[:, 0], found on the device."""
    device = engine._require_gpu(t.device if torch.is_tensor(t) and t.is_cuda else device)
    tgt = _int_ids(target_idx_l, "segment_rank_fil_device", "target_idx_l")
    B = len(tgt)
    scores = torch.as_tensor(t).detach().to(device=device, dtype=torch.float32).contiguous()
    ents = torch.as_tensor(entities).to(device)
    if ents.dim() != 2 or ents.shape[1] != 2 or ents.shape[0] != scores.numel():
        raise ValueError("segment_rank_fil_device: entities must be [N, 2] with one row per score (got %s for %d scores)"
                         % (tuple(ents.shape), scores.numel()))
    seg = ents[:, 0]
    starts = torch.nonzero(seg[1:] != seg[:-1]).reshape(-1) + 1
    seg_ptr = torch.cat([starts.new_zeros(1), starts, starts.new_full((1,), len(seg))])
    if seg_ptr.numel() != B + 1:
        raise ValueError("segment_rank_fil_device: %d segments for %d targets" % (seg_ptr.numel() - 1, B))
    sub, pre, ts = (_int_ids(x, "segment_rank_fil_device", k) for x, k in ((queries_sub, "queries_sub"), (queries_pre, "queries_pre"),
                                                                            (queries_ts, "queries_ts")))
    keys = [None if ix is None else torch.as_tensor(ix.query_keys(sub, pre, ts)).to(device) for ix in (sp_index, spt_index)]
    known = [None if ix is None else _index_tensors(ix, device) for ix in (sp_index, spt_index)]
    out = engine.segment_rank(scores, ents[:, 1].to(torch.int32).contiguous(), seg_ptr, torch.as_tensor(tgt, dtype=torch.int32).to(device),
                              keys[0], known[0], keys[1], known[1])
    rank, rank_fil, rank_fil_t, found = torch.stack([x.float() for x in out]).cpu().numpy().astype(np.float64)
    found = found != 0
    return rank, found.tolist(), rank_fil, rank_fil_t[found]


def extrapolation_metrics(rank, found, rank_fil, rank_fil_t):
    """The reference's reported quantities (main.py:413-430,434-463) from the ranks of a split: ``rank`` / ``rank_fil`` [n] (1e9 where not
    found), ``found`` bool [n], ``rank_fil_t`` over the found queries only, as segment_rank_fil leaves them.  Sums in float64."""
    rank, rank_fil, rank_fil_t = (np.asarray(x, dtype=np.float64) for x in (rank, rank_fil, rank_fil_t))
    found = np.asarray(found, dtype=bool)
    n, n_found = len(rank), int(found.sum())
    among = lambda v: float(v) / n_found if n_found else float("nan")
    return {
        "n": n, "n_found": n_found,
        "hits1": np.sum(rank == 1) / n, "hits3": np.sum(rank <= 3) / n, "hits10": np.sum(rank <= 10) / n,
        "hits_inf": n_found / n, "mr": np.sum(rank) / n, "mrr": np.sum(1 / rank) / n,
        "hits1_fil": np.sum(rank_fil <= 1) / n, "hits3_fil": np.sum(rank_fil <= 3) / n, "hits10_fil": np.sum(rank_fil <= 10) / n,
        "mrr_fil": np.sum(1 / rank_fil) / n,
        "hits1_fil_t": np.sum(rank_fil_t <= 1) / n, "hits3_fil_t": np.sum(rank_fil_t <= 3) / n, "hits10_fil_t": np.sum(rank_fil_t <= 10) / n,
        "mrr_fil_t": np.sum(1 / rank_fil_t) / n,
        "hits1_found": among(np.sum(rank == 1)), "hits3_found": among(np.sum(rank <= 3)), "hits10_found": among(np.sum(rank <= 10)),
        "mr_found": among(np.sum(rank[found])), "mrr_found": among(np.sum(1 / rank[found])),
    }
