"""T_RED_GNN (temporal interpolation) with the reference's parameter names, on the HIP path (inference).

Mirrors Temporal/interpolation/model_cuda.py:21-213: per-layer relation tables ``rela_embed_layer.{i}``,
``attention_1_layer.{i}`` (Linear(3d -> a), no bias), ``attention_2_layer.{i}`` (Linear(a -> 1), no bias),
``past_linear / now_linear / future_linear`` (d x d, no bias), ``time_embed`` (n_time x d), ``linear_classifier``
(d -> 1 with bias); ``score_embed_layer`` and ``query_relation_linear`` exist in the reference's state dict but are
unused by its forward (model_cuda.py:210) and are kept for checkpoint compatibility.  ``shared_tables=True`` gives the
parameter layout of Temporal/interpolation/model.py (one rela_embed / attention_1 / attention_2 for all layers).

What is different inside: the per-call scipy coo build, the dense [B, n_ent] index maps and the python
attention_vis loop with .item() syncs (model_cuda.py:121-135,163-166,178-184) do not exist; frontier expansion is the
device bitmap walk, and the per-edge work of a layer is one fused kernel (rg_tlayer_fwd) with the three direction linears
hoisted per node / relation / |dt| (W(h + r + tau) = Wh + Wr + Wtau).  The attention_vis table itself - alpha sum and edge count per
relation - is ``attention_profile`` (rg_tattn_profile; with the edge direction past / now / future as one more axis), the r-digraph the
reference draws in model_cuda_rule_vis.py is ``explain`` (rg_texplain_*; every edge with its time id), ``rules`` / ``rules_all`` count
its best paths as temporal rules, ``rule_quality`` counts how those hold in the quadruple graph (rg_trule_ground), ``rule_scores`` /
``rule_predict`` / ``rule_evaluate`` apply them to queries (rg_trule_apply: what the rules alone predict, and how well), ``fidelity`` /
``fidelity_all`` re-score an answer on its r-digraph without, and with only, its best paths' quadruples (rg_digraph_tlayer_fwd), and ``predict`` gives the
filtered top-k answers of (head, relation, time) queries (rg_topk).  The validation loop of main.py:125-183 is ``evaluate`` /
``rank_batch`` (evaluation.py, rg_segment_eval): loss, raw and filtered ranks from the visited pairs, without the [B, n_ent] matrix.
Training: ``mode='train'`` drops the batch's own quadruples (``batch['example_idx']`` rows of ``params.graph``,
model_cuda.py:103-104) by building a device graph for the batch, applies ``nn.Dropout(params.dropout)`` before the
activation (:196) and is differentiable: the per-edge work of the backward pass is rg_tlayer_bwd, the hoisted linears are
ordinary autograd GEMMs.
"""
import contextlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import engine
from .models import pad_attn, tall_linear


def _pad4(n):
    return (n + 3) // 4 * 4


class _TAggregate(torch.autograd.Function):
    """agg = rg_tlayer_fwd(...);  backward = rg_tlayer_bwd(...)."""

    @staticmethod
    def forward(ctx, hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha, b_alpha, lease, graph, level, n_new, q_time,
                d, attn_dim):
        hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha = (t.contiguous() for t in (hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha))
        agg = engine.tlayer_fwd(lease.frontier, graph, level, n_new, q_time, hidden_dir, rela_dir, time_dir, d, a_s, a_r, a_q,
                                w_alpha, b_alpha, attn_dim)
        ctx.save_for_backward(hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha, b_alpha, q_time)
        ctx.misc = (lease, graph, level, d, attn_dim)      # the lease keeps the frontier's level bitmaps for this graph's backward
        return agg

    @staticmethod
    def backward(ctx, grad_agg):
        hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha, b_alpha, q_time = ctx.saved_tensors
        lease, graph, level, d, attn_dim = ctx.misc
        lease.check()
        g_hd, g_rd, g_td, g_as, g_ar, g_aq, g_w = engine.tlayer_bwd(lease.frontier, graph, level, a_s.shape[0], q_time, hidden_dir, rela_dir,
                                                              time_dir, d, a_s, a_r, a_q, w_alpha, b_alpha, attn_dim, grad_agg)
        if level == 1:
            lease.release()
        return (g_hd, g_rd, g_td, g_as, g_ar, g_aq, g_w.view_as(w_alpha)) + (None,) * 8


class T_RED_GNN(nn.Module):
    def __init__(self, params, shared_tables=False):
        super().__init__()
        self.n_rel, self.n_ent, self.n_time = params.n_rel, params.n_ent, params.n_time      # n_rel: relation ids in the graph (incl. idd)
        self.hidden_dim, self.attn_dim, self.n_layer = params.hidden_dim, params.attn_dim, params.n_layer
        self.shared_tables = shared_tables
        d, a = self.hidden_dim, self.attn_dim
        if shared_tables:       # Temporal/interpolation/model.py:19-21
            self.rela_embed = nn.Embedding(self.n_rel + 1, d)
            self.attention_1 = nn.Linear(3 * d, a, bias=False)
            self.attention_2 = nn.Linear(a, 1, bias=False)
        else:                   # Temporal/interpolation/model_cuda.py:32-35
            self.rela_embed_layer = nn.ModuleList([nn.Embedding(self.n_rel + 1, d) for _ in range(self.n_layer)])
            self.score_embed_layer = nn.Embedding(self.n_rel + 1, d)
            self.attention_1_layer = nn.ModuleList([nn.Linear(3 * d, a, bias=False) for _ in range(self.n_layer)])
            self.attention_2_layer = nn.ModuleList([nn.Linear(a, 1, bias=False) for _ in range(self.n_layer)])
            self.query_relation_linear = nn.Linear(d, 1, bias=False)
        self.linear_classifier = nn.Linear(d, 1)
        self.past_linear = nn.Linear(d, d, bias=False)
        self.now_linear = nn.Linear(d, d, bias=False)
        self.future_linear = nn.Linear(d, d, bias=False)
        self.time_embed = nn.Embedding(self.n_time, d)
        acts = {"tanh": torch.tanh, "sigmoid": torch.sigmoid, "relu": torch.relu, "idd": lambda x: x,
                "softplus": F.softplus, "leaky_relu": F.leaky_relu}
        self.act = acts[params.act]
        self.dropout = nn.Dropout(getattr(params, "dropout", 0.0))               # model_cuda.py:58
        self.quads = np.ascontiguousarray(np.asarray(params.graph, dtype=np.int32).reshape(-1, 4))
        self.graph = engine.TemporalGraph(self.n_ent, self.n_rel + 1, self.n_time, self.quads,
                                          device=getattr(params, "device", "cuda"))
        self._frontiers = engine.FrontierPool()
        self.last_stats = None

    def _tables(self, i):
        if self.shared_tables:
            return self.rela_embed.weight, self.attention_1.weight, self.attention_2.weight
        return self.rela_embed_layer[i].weight, self.attention_1_layer[i].weight, self.attention_2_layer[i].weight

    def _frontier(self, n, n_levels, device):
        return self._frontiers.get(self.n_ent, n, n_levels, device)

    def forward(self, batch, mode="train"):
        return self._run(batch, mode)

    def explain(self, batch, objs=None, min_alpha=0.0):
        """The r-digraph behind the answer objs[b] of every query (head, relation, time) of ``batch`` (the dict forward takes), on the
        full graph (mode="test": no fact is deleted), under no_grad: explain.RDigraph with ``time`` (the time id of every edge) and
        ``q_time`` set.  objs=None: the model's own top answer per row.  Edges with attention below min_alpha are left out."""
        from . import explain as _explain
        return _explain.explain_temporal(self, batch, objs, min_alpha)

    def rules(self, batch, objs=None, k=1, min_alpha=0.0):
        """The k best paths behind the answer of every query of ``batch`` counted as temporal rules: explain -> top_paths(k) ->
        explain.TemporalRuleTable, one row per distinct (query relation, (relation, direction) of every step), the direction being
        the forward's past / now / future of the step's edge against the query time and identity steps written as "any".  objs=None:
        batch["tail"] where the batch has it, else the model's own top answer per row, as explain."""
        from . import explain as _explain
        if objs is None and "tail" in batch:
            objs = batch["tail"]
        rd = self.explain(batch, objs, min_alpha)
        return _explain.temporal_rules_from_paths(rd.top_paths(k), batch["relation"], self.n_rel)

    def rules_all(self, quads, k=1, batch_size=64):
        """The rule tables of ``quads`` int [n, 4] = (head, rel, tail, time id), the layout of params.graph - each row a query with its
        tail as the answer - walked in batches of ``batch_size`` rows and added (tables add exactly)."""
        q = np.asarray(quads.detach().cpu().numpy() if torch.is_tensor(quads) else quads)
        if q.ndim != 2 or q.shape[1] != 4 or len(q) == 0 or q.dtype == np.bool_ or not np.issubdtype(q.dtype, np.integer):
            raise ValueError("rules_all: quads must be a non-empty integer array [n, 4] = (head, rel, tail, time id) (got %s %s)"
                             % (q.dtype, q.shape))
        if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
            raise ValueError("rules_all: batch_size must be a positive integer (got %r)" % (batch_size,))
        table = None
        for lo in range(0, len(q), int(batch_size)):
            part = q[lo:lo + int(batch_size)]
            t = self.rules({"head": part[:, 0], "relation": part[:, 1], "time": part[:, 3]}, part[:, 2], k=k)
            table = t if table is None else table + t
        return table

    def fidelity(self, batch, objs=None, k=4, inverse_offset=None):
        """How much of each answer's score its best paths carry, as RED_GNN_trans.fidelity: one explain, one top_paths(k) and 2k
        RDigraph.rescore calls (rg_digraph_tlayer_fwd per hop, no graph rebuild) - the answers re-scored without the quadruples of the
        row's best j paths (``without``) and with those quadruples and the identity edges alone (``only``), j = 1..k: an
        explain.Fidelity.  objs=None: batch["tail"] where the batch has it, else the model's own top answer per row, as rules.
        ``inverse_offset`` = m: a quadruple is deleted together with its inverse twin (t, r + m if r < m else r - m, h, time id), the
        way the data wrote its inverses (m = the number of base relations for the reference's loaders); None: only the quadruples
        the paths step over."""
        from . import explain as _explain
        return _explain.temporal_fidelity(self, batch, objs, k, inverse_offset)

    def saliency(self, batch, objs=None):
        """How much the score of each answer depends on every quadruple of its r-digraph, in one pass: ``explain`` followed by
        RDigraph.saliency - the gradient of the score with respect to a gate on every edge's message (the timed edge-list layer's
        adjoint in HIP, rg_digraph_tlayer_bwd).  Returns an explain.Saliency: ``edge_grad`` per edge of ``.digraph``, ``fact_grad()`` /
        ``top(k)`` per quadruple (h, r, t, time id), ``deletion_estimate(mask)`` the first-order estimate of a rescore.  objs=None: the
        model's own top answer per row, as explain.  Eval semantics; the parameters get no gradient."""
        return self.explain(batch, objs).saliency(self)

    def fidelity_all(self, quads, k=4, batch_size=64, inverse_offset=None):
        """fidelity over ``quads`` int [n, 4] = (head, rel, tail, time id), each row a query with its tail as the answer, walked in
        batches of ``batch_size`` rows: the dict BaseModel.fidelity returns (n, k, necessity_mean / _median, sufficiency_gap_mean /
        _median, disconnected, each a list over j = 1..k)."""
        from . import explain as _explain
        return _explain.temporal_fidelity_all(self, quads, k, batch_size, inverse_offset)

    def rule_quality(self, table, anchors=None, scratch_bytes=engine.RULE_SCRATCH_BYTES):
        """How the rules of ``table`` (an explain.TemporalRuleTable) hold in the full quadruple graph, the one explain walks:
        explain.TemporalRuleQuality with the exact counts body_pairs, hits, pca_body_pairs and head_pairs of every rule over the pairs
        ((x, t), y), (x, t) an anchor - ``anchors`` int [S, 2] = (entity, time id), distinct; None: every (head, time) of the graph's
        non-identity rows - counted in HIP (rg_trule_ground), independent of ``scratch_bytes``, which bounds the bitmaps of a chunk.

        The counts are taken on the graph as built, so ``hits`` says how often a rule reproduces facts the graph already holds.  A
        table mined from quadruples that are in the graph (the training set) contains, for each of them, the trivial rule "the fact
        itself, now" with confidence 1 (``trivial()`` marks it): mine on held-out quadruples."""
        from . import explain as _explain
        if not isinstance(table, _explain.TemporalRuleTable):
            raise ValueError("rule_quality: table must be an explain.TemporalRuleTable (got %s)" % type(table).__name__)
        if table.n_rel != self.n_rel:
            raise ValueError("rule_quality: the table has n_rel=%d, the model n_rel=%d" % (table.n_rel, self.n_rel))
        counts = engine.trule_ground(self.graph, table.head, table.body, table.direction, anchors, scratch_bytes)
        n_anchors = len(self.graph.default_anchors()) if anchors is None else int(len(anchors))
        return _explain.TemporalRuleQuality(table, *(counts[:, c].contiguous() for c in range(4)), n_anchors)

    def rule_scores(self, quality, batch, by="confidence", laplace=0.0, min_hits=1, drop_trivial=True,
                    scratch_bytes=engine.RULE_SCRATCH_BYTES):
        """What the rules of ``quality`` (an explain.TemporalRuleQuality, from rule_quality) predict for the queries (head, relation,
        ?, time) of ``batch`` (the dict forward takes) on the full quadruple graph, in HIP (rg_trule_apply): explain.RuleScores with
        best / surv / best_rule / fired [B, n_ent].  A rule fires for (b, y) iff its head is the query relation and its steps lead
        from the head to y through rows whose time stands to the query's as each step's direction says.  The rules kept and their
        weights are explain.rule_weights(quality, by, laplace, min_hits, drop_trivial); ``best_rule`` holds table rows.  No bit
        depends on ``scratch_bytes``, which bounds the bitmaps of one call."""
        from . import explain as _explain
        return _explain.temporal_rule_scores(self, quality, batch, by, laplace, min_hits, drop_trivial, scratch_bytes)

    def rule_predict(self, quality, batch, k=10, agg="noisy_or", known=None, **weights):
        """The k best answers of every query of ``batch`` by rule score alone (agg "noisy_or": 1 - the product of the firing rules'
        1 - weight; "max": the largest weight), selected in HIP (rg_topk): explain.RulePrediction, score descending then entity id
        ascending, -1 / -inf / -1 / 0 past the end, ``rule`` the table row of each answer's best rule and ``table`` the
        TemporalRuleTable, so format() prints the rule with its [past] / [now] / [future] tags.  ``known`` =
        prediction.temporal_known_index(...): the tails it lists for a query's (head, relation, time) are left out.  ``weights``:
        by, laplace, min_hits, drop_trivial, scratch_bytes of rule_scores.  A batch without rows gives [0, k] tensors."""
        from . import explain as _explain
        return _explain.temporal_rule_predict(self, quality, batch, k, agg, known, **weights)

    def rule_evaluate(self, quads, quality=None, mine=None, k=1, agg="noisy_or", known=None, known_static=None, batch_size=256,
                      **weights):
        """Ranking metrics of the rules alone on ``quads`` int [n, 4] = (head, rel, tail, time id), next to evaluate: exactly one of
        ``quality`` (a TemporalRuleQuality) and ``mine`` (int [m, 4] quadruples, e.g. the valid split: rules_all(mine, k) ->
        rule_quality) is given.  Per batch of ``batch_size`` queries the rule scores (rule_scores, ``agg``) are ranked by rg_rank three
        times - raw, with the time-aware filter ``known`` = prediction.temporal_known_index(...) and with the static filter
        ``known_static`` = prediction.temporal_static_known_index(...); a query's filter set is its tail and the tails the index
        lists for its key.  Returns a dict: n, coverage (the share of tails some rule reaches) and hits1 / hits3 / hits10 / mrr / mr
        with the suffixes "" / _fil_t / _fil of evaluate, sums in float64.

        One difference from evaluate: rg_rank's tie term counts every entity that scores exactly as the tail, filtered ones
        included, where rg_segment_eval's eq_fil leaves the filtered ones out.  Every entity no rule reaches scores 0, so the
        filtered rank of an unreached tail is larger here by half the number of filtered entities that are unreached too.  The
        convention is BaseModel.rule_evaluate's."""
        from . import explain as _explain
        return _explain.temporal_rule_evaluate(self, quads, quality, mine, k, agg, known, known_static, batch_size, **weights)

    def attention_profile(self, batch, group="relation"):
        """Edge count and alpha sum per (query | query relation, hop, direction, edge relation) over the hop edges of the queries of
        ``batch``, on the full graph, under no_grad: profile.AttentionProfile with axes ("group", "hop", "direction", "relation"),
        direction 0 past / 1 now / 2 future of the edge's time against the query's.  ``collapse("direction")`` is the table the
        reference's attention_vis holds."""
        from . import profile as _profile
        return _profile.attention_profile_temporal(self, batch, group)

    def predict(self, batch, k=10, known=None):
        """The k best answers of every query of ``batch`` on the full graph, under no_grad: prediction.Prediction, score descending then
        entity id ascending, -1 / -inf past the end.  ``known`` = prediction.temporal_known_index(...) (numpy or device tensors): the
        tails it lists for a query's (head, relation, time) are left out; None excludes nothing."""
        from . import prediction as _prediction
        return _prediction.predict_temporal(self, batch, k, known)

    def rank_batch(self, batch, tails=None, known=None, known_static=None):
        """Loss term and ranks of one batch as the validation loop of main.py:140-164 computes them, on the device and without the
        [B, n_ent] matrix: the forward on the full graph, then rg_segment_eval on its visited pairs.  ``batch`` is forward's dict;
        ``tails`` int [B] defaults to batch["tail"].  ``known`` = prediction.temporal_known_index(...) hides the other known tails
        of a query's (head, relation, time) - the time-aware filter - and ``known_static`` =
        prediction.temporal_static_known_index(...) those of its (head, relation); numpy triples or device tensors, None filters
        nothing.  No gradients, eval mode (the training flags come back).  Returns evaluation.TemporalRanks."""
        from . import evaluation as _evaluation
        return _evaluation.rank_batch_temporal(self, batch, tails, known, known_static)

    def evaluate(self, quads, known=None, known_static=None, batch_size=64, return_ranks=False):
        """Loss and ranking metrics of ``quads`` int [n, 4] = (head, rel, tail, time id), the layout of params.graph, in batches of
        ``batch_size`` through rank_batch; the results stay on the device and are copied to the host once.  Returns a dict: n, loss
        (mean of -logp), unreached (share of targets the forward never visited), and hits1 / hits3 / hits10 / mrr / mr raw, *_fil_t
        (time-aware filter, ``known``) and *_fil (static filter, ``known_static``), sums in float64.  ``return_ranks`` adds
        "per_query": the numpy arrays logp, visited, gt / eq, gt_fil_t / eq_fil_t, gt_fil / eq_fil and rank, rank_fil_t, rank_fil.

        Relation to the reference: ``loss`` is main.py:146,170.  Its own rank (main.py:161-163, an argsort) and hits (util.py:42-51,
        topk) place a tied answer at any of the tied places - and every unreached entity scores exactly 0, so ties are the normal
        case; they always lie in [gt + 1, gt + eq + 1].  This method reports the mean of that interval, gt + eq / 2 + 1, the
        convention of rg_rank and rg_segment_rank.  The reference has no filtered metric."""
        from . import evaluation as _evaluation
        return _evaluation.evaluate_temporal(self, quads, known, known_static, batch_size, return_ranks)

    def _run(self, batch, mode, kept=None, dense=True):
        """forward(); with ``kept`` (a list) the frontier keeps all n_layer + 1 levels and the list receives dict(frontier, graph, q_rel,
        q_time) followed per layer by dict(a_s [n_old, ap], a_r [n_rel + 1, ap], a_q [B, ap], w_alpha [attn_dim]): what rg_tlayer_fwd
        read, for rg_texplain_* and rg_tattn_profile.  dense=False: (result fp32 [N], nodes int32 [N, 2]) - the logit of every visited
        (query, entity) pair, sorted by query then entity - instead of the [B, n_ent] matrix, which is then never built."""
        device = self.linear_classifier.weight.device
        engine._require_gpu(device)
        heads = torch.as_tensor(batch["head"]).to(device=device, dtype=torch.int32)
        q_rel = torch.as_tensor(batch["relation"]).to(device=device, dtype=torch.int64)
        q_time = torch.as_tensor(batch["time"]).to(device=device, dtype=torch.int32)
        n = heads.numel()
        graph = self.graph
        if mode == "train":     # model_cuda.py:103-104: the batch's own facts leave the graph
            drop = np.asarray(torch.as_tensor(batch["example_idx"]).cpu()).reshape(-1)
            graph = engine.TemporalGraph(self.n_ent, self.n_rel + 1, self.n_time, self.quads, device=device, exclude=drop)
        with_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        fr = self._frontier(n, self.n_layer + 1 if (with_grad or kept is not None) else 2, device)
        fr.reset(heads)
        if kept is not None:
            kept.append(dict(frontier=fr, graph=graph, q_rel=q_rel, q_time=q_time))
        lease = engine.FrontierLease(fr) if with_grad else None
        d, a = self.hidden_dim, self.attn_dim
        ld, ap = max(16, _pad4(d)), pad_attn(a)
        w_dir = torch.cat([self.past_linear.weight, self.now_linear.weight, self.future_linear.weight], 0)     # [3d, d]
        padc = lambda t: F.pad(t, (0, ld - d)) if ld != d else t
        pad_rows = lambda w: F.pad(w, (0, 0, 0, ap - a)) if ap != a else w
        time_dir = padc(F.linear(self.time_embed.weight, w_dir).view(self.n_time, 3, d).transpose(0, 1).reshape(3 * self.n_time, d)).contiguous()
        hidden = torch.zeros((n, d), device=device)
        zero_b = torch.zeros(1, device=device)
        n_edges, nodes = [], None
        for i in range(self.n_layer):
            rela, w1, w2 = self._tables(i)
            n_new, n_e, n_old = fr.expand(graph)
            n_edges.append(n_e)
            if with_grad:
                engine.prefer_blas(n_new)
            a_s = tall_linear(hidden, pad_rows(w1[:, :d])).contiguous()               # [n_old, ap]
            a_r = F.linear(rela, pad_rows(w1[:, d:2 * d])).contiguous()              # [n_rel+1, ap]
            a_q = F.linear(rela[q_rel], pad_rows(w1[:, 2 * d:])).contiguous()        # [B, ap]
            hidden_dir = padc(tall_linear(hidden, w_dir).view(n_old * 3, d)).contiguous()        # row 3 s + dir
            rela_dir = padc(F.linear(rela, w_dir).view(-1, 3, d).transpose(0, 1).reshape(-1, d)).contiguous()   # row dir*(R+1) + r
            w_alpha = w2.reshape(-1).contiguous()
            if kept is not None:
                kept.append(dict(a_s=a_s, a_r=a_r, a_q=a_q, w_alpha=w_alpha))
            if with_grad:
                agg = _TAggregate.apply(hidden_dir, rela_dir, time_dir, a_s, a_r, a_q, w_alpha, zero_b, lease, graph, fr.level, n_new,
                                        q_time, d, a)
            else:
                with torch.no_grad():
                    agg = engine.tlayer_fwd(fr, graph, fr.level, n_new, q_time, hidden_dir, rela_dir, time_dir, d, a_s, a_r, a_q,
                                            w_alpha, zero_b, a)
            hidden = self.act(self.dropout(agg[:, :d]))                               # model_cuda.py:196
        nodes, _, _ = fr.nodes(want_prev=False, want_old_new=False)
        result = tall_linear(hidden, self.linear_classifier.weight, self.linear_classifier.bias).reshape(-1)   # model_cuda.py:210
        self.last_stats = dict(n_edges=n_edges, n_nodes=int(nodes.shape[0]))
        self.last_nodes = nodes
        if not dense:
            return result, nodes
        key_idx = nodes[:, 0].long() * self.n_ent + nodes[:, 1].long()
        score_all = torch.zeros(n * self.n_ent, device=device).index_copy(0, key_idx, result)
        return score_all.view(n, self.n_ent)


@contextlib.contextmanager
def eval_semantics(model):
    """The module in eval mode (dropout = identity) for the duration, whatever its mode: explain, attention_profile and predict
    describe the deterministic model.  Every submodule gets its own flag back."""
    was = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        yield
    finally:
        for m, flag in was:
            m.training = flag


def batch_ids(model, batch, who):
    """(head, relation, time) of ``batch`` as int64 numpy arrays, validated against the model's id ranges."""
    def ids(k):
        if k not in batch:
            raise ValueError("%s: the batch needs 'head', 'relation' and 'time' (missing %r)" % (who, k))
        x = batch[k]
        a = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).reshape(-1)
        if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):      # (no silent truncation of 1.7 to 1)
            raise ValueError("%s: batch[%r] must hold integer ids (got dtype %s)" % (who, k, a.dtype))
        return a.astype(np.int64)
    h, r, t = ids("head"), ids("relation"), ids("time")
    n = len(h)
    if n == 0 or len(r) != n or len(t) != n:
        raise ValueError("%s: need one relation and one time per head and at least one row (got %d heads, %d relations, %d times)"
                         % (who, n, len(r), len(t)))
    if h.min() < 0 or h.max() >= model.n_ent or r.min() < 0 or r.max() > model.n_rel or t.min() < 0 or t.max() >= model.n_time:
        raise ValueError("query head / relation / time id out of range (n_ent=%d, n_rel+1=%d, n_time=%d)"
                         % (model.n_ent, model.n_rel + 1, model.n_time))
    return h, r, t

