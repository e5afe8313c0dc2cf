"""The relational digraph (r-digraph) behind an answer, with its attention weights.

For a query (s, r) and an answer o, RED-GNN's score of o depends only on the edges of the union of all length-L relational paths
s -> o through the query's subgraph (identity self-loops count as steps); each edge carries its layer's attention alpha.

    rd = model.explain(subs, rels, objs)            # objs=None: the model's own top answer per row
    rd.edges[rd.offsets[b]:rd.offsets[b + 1]]       # (row, hop, head, rel, tail) of row b, hop 1..L
    rels_, ents, prod = rd.strongest_paths()         # the path of largest alpha product per row

The extraction runs in HIP (csrc/explain.hip): a forward keeps all L + 1 frontier levels and each layer's attention projection, then
one backward marking pass per hop reads only the marked tails' CSR rows.  This module holds the result type and the host drivers.

Temporal interpolation (T_RED_GNN.explain, rg_texplain_*): ``rd = model.explain(batch, objs)`` with the batch dict of forward; every
edge also carries its time id (``rd.time``), ``rd.q_time`` is the rows' query time and ``rd.direction()`` the forward's past / now /
future of each edge.

Temporal extrapolation (extrapolation.T_RED_GNN.explain, rg_xexplain_*): ``rd = model.explain(X, objs)`` with the batch object of
forward; ``rd.data_row`` names the past fact behind every edge (-1: a self-loop, relation id n_rel), ``rd.time`` its day and
``rd.lag()`` how many days before the query it lies.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import engine
from .models import _pad4, pad_attn


@dataclass
class RDigraph:
    """r-digraphs of a batch of rows (s, r, o).  Tensors on the device that computed them.

    edges    int32 [E, 5]  (row, hop, head, rel, tail), hop in 1..L, ordered by (row, hop, tail, position of the edge in the graph's
                           CSR by tail = fact-row order)
    alpha    float32 [E]   attention of the edge in its layer
    offsets  int64 [B+1]   edges of row b: offsets[b]:offsets[b+1]
    reached  bool [B]      o is in the query's level-L node set
    score    float32 [B]   the model's score of o (0 where not reached)
    n_hops   int           L
    time     int32 [E]     temporal models only (None otherwise): the time id of each edge; a fact repeated at several times is one
                           edge per time, in CSR order
    q_time   int32 [B]     temporal models only (None otherwise): the query time of each row
    data_row int32 [E]     extrapolation only (None otherwise): the edge's index into the model's data array, -1 for a self-loop;
                           there ``time`` is the day the forward used for the edge (the row's day; a self-loop's: the first day of
                           the row's window) and ``q_time`` the query's day
    """
    edges: torch.Tensor
    alpha: torch.Tensor
    offsets: torch.Tensor
    reached: torch.Tensor
    score: torch.Tensor
    n_hops: int
    time: torch.Tensor = None
    q_time: torch.Tensor = None
    data_row: torch.Tensor = None

    def direction(self):
        """int8 [E]: each edge's direction against its row's query time, the temporal forward's convention (dt = edge time - query
        time): 0 past (dt < 0), 1 now (dt == 0), 2 future (dt > 0).  Temporal digraphs only."""
        if self.time is None or self.q_time is None:
            raise ValueError("direction: a static r-digraph has no edge times")
        dt = self.time.long() - self.q_time.long()[self.edges[:, 0].long()]
        return (dt > 0).to(torch.int8) * 2 + (dt == 0).to(torch.int8)

    def lag(self):
        """int32 [E]: query time of the edge's row - edge time, the row of the relative-time table the extrapolation forward read for
        the edge.  Temporal digraphs only."""
        if self.time is None or self.q_time is None:
            raise ValueError("lag: a static r-digraph has no edge times")
        return self.q_time[self.edges[:, 0].long()] - self.time

    def strongest_paths(self):
        """Per row, the length-L path s -> o inside the digraph with the largest product of alpha (products in float64, left to right
        from s; the best prefix is kept per node and level).  Ties go to the smallest (head, rel) at each step, taken from o backwards.
        Returns (rel ids int64 [B, L], entity ids int64 [B, L+1] from s to o, product float64 [B]); rows without edges: -1 and 0.
        Works on the compact edge list (device or CPU tensors)."""
        B, L = self.offsets.numel() - 1, self.n_hops
        dev = self.edges.device
        rels_out = torch.full((B, L), -1, dtype=torch.int64, device=dev)
        ents_out = torch.full((B, L + 1), -1, dtype=torch.int64, device=dev)
        prod_out = torch.zeros(B, dtype=torch.float64, device=dev)
        if self.edges.shape[0] == 0:
            return rels_out, ents_out, prod_out
        e = self.edges.long()
        a = self.alpha.double()
        row, hop, head, rel, tail = e.unbind(1)
        n_key = int(torch.maximum(head.max(), tail.max()).item()) + 1
        keys, best, cand = [None] * (L + 1), [None] * (L + 1), [None] * (L + 1)
        for l in range(1, L + 1):                        # forward: best prefix product per (row, node) of level l
            m = hop == l
            hk = row[m] * n_key + head[m]
            if l == 1:
                pre = torch.ones(hk.numel(), dtype=torch.float64, device=dev)
            else:
                pos = torch.searchsorted(keys[l - 1], hk).clamp_(max=max(keys[l - 1].numel() - 1, 0))
                ok = keys[l - 1][pos] == hk
                pre = torch.where(ok, best[l - 1][pos], torch.zeros_like(a[m]))
            cand[l] = pre * a[m]
            tk = row[m] * n_key + tail[m]
            keys[l], inv = torch.unique(tk, sorted=True, return_inverse=True)
            best[l] = torch.zeros(keys[l].numel(), dtype=torch.float64, device=dev).scatter_reduce(0, inv, cand[l], "amax",
                                                                                                   include_self=False)
        # backward from o: at each hop the in-edge of the current node with the best candidate product, smallest (head, rel) on a tie
        cur = torch.full((B,), -1, dtype=torch.int64, device=dev)
        for l in range(L, 0, -1):
            m = hop == l
            r_, h_, rl_, t_, c_ = row[m], head[m], rel[m], tail[m], cand[l]
            sel = (t_ == cur[r_]) if l < L else torch.ones_like(r_, dtype=torch.bool)
            if l == L:
                ents_out[r_, L] = t_                     # every hop-L edge of a row ends at its o
                prod_out[r_] = 0.0
            r_, h_, rl_, c_ = r_[sel], h_[sel], rl_[sel], c_[sel]
            order = torch.argsort(rl_, stable=True)
            for k in (h_, -c_, r_):
                order = order[torch.argsort(k[order], stable=True)]
            r_, h_, rl_, c_ = r_[order], h_[order], rl_[order], c_[order]
            first = torch.ones_like(r_, dtype=torch.bool)
            first[1:] = r_[1:] != r_[:-1]
            r_, h_, rl_, c_ = r_[first], h_[first], rl_[first], c_[first]
            if l == L:
                prod_out[r_] = c_
            rels_out[r_, l - 1] = rl_
            ents_out[r_, l - 1] = h_
            cur = torch.full((B,), -1, dtype=torch.int64, device=dev)
            cur[r_] = h_
        none = ents_out[:, 0] < 0
        rels_out[none] = -1
        ents_out[none] = -1
        prod_out[none] = 0.0
        return rels_out, ents_out, prod_out


def _ids(x, name):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a.astype(np.int64).reshape(-1)


def explain(model, subs, rels, objs=None, mode="test", min_alpha=0.0):
    """RED_GNN_trans.explain (see there)."""
    device = model.W_final.weight.device
    engine._require_gpu(device)
    subs_h, rels_h = _ids(subs, "subs"), _ids(rels, "rels")
    n = len(subs_h)
    if n == 0 or len(rels_h) != n:
        raise ValueError("explain: need one relation per subject and at least one row (got %d subjects, %d relations)" % (n, len(rels_h)))
    graph = model.loader.graph_for(mode)
    n_ent = graph.n_ent
    if subs_h.min() < 0 or subs_h.max() >= n_ent or rels_h.min() < 0 or rels_h.max() > 2 * model.n_rel:
        raise ValueError("query subject / relation id out of range (n_ent=%d, 2*n_rel+1=%d)" % (n_ent, 2 * model.n_rel + 1))
    objs_h = None
    if objs is not None:
        objs_h = _ids(objs, "objs")
        if len(objs_h) != n:
            raise ValueError("explain: %d answers for %d rows" % (len(objs_h), n))
        if objs_h.min() < 0 or objs_h.max() >= n_ent:
            raise ValueError("answer id out of range (n_ent=%d)" % n_ent)
    tau = float(min_alpha)
    if tau != tau:
        raise ValueError("explain: min_alpha is NaN")
    L = model.n_layer
    d, a = model.hidden_dim, model.attn_dim
    ld, ap = max(16, _pad4(d)), pad_attn(a)
    with torch.no_grad():
        kept = []
        scores = model._run(subs_h, rels_h, mode, kept=kept)
        fr, q_rel = kept[0]["frontier"], kept[0]["q_rel"]
        layers = kept[1:]
        tables = [k["tables"] for k in layers]
        if any(t is None for t in tables):
            tables = model.inference_tables(q_rel, ld, ap)
        if objs_h is None:
            objs_t = scores.argmax(1)                    # first maximum = smallest entity id on a tie
        else:
            objs_t = torch.as_tensor(objs_h, dtype=torch.int64).to(device)
        marks, reached = engine.explain_seed(fr, L, objs_t.to(torch.int32).contiguous())
        hops = [None] * (L + 1)
        for l in range(L, 0, -1):
            layer = model.gnn_layers[l - 1]
            a_r, a_q, _ = tables[l - 1]
            a_s = layers[l - 1]["a_s"].detach().contiguous()
            marks, e, al = engine.explain_hop(fr, graph, l, marks, a_s, a_r.contiguous(), a_q.contiguous(),
                                              layer.w_alpha.weight.detach().reshape(-1).contiguous(),
                                              layer.w_alpha.bias.detach().contiguous(), a, tau)
            hops[l] = (e, al)
        if tau > 0.0:
            hops = _forward_sweep(hops, L, n_ent)
        rows = torch.arange(n, device=device)
        score = scores[rows, objs_t].contiguous()
        edges, alpha, offsets, _ = _assemble(hops, n, L, device)
    return RDigraph(edges=edges, alpha=alpha, offsets=offsets, reached=reached, score=score, n_hops=L)


def _assemble(hops, n, L, device):
    """The hops' lists hops[l] = (edges [E_l, 4], alpha [E_l][, time [E_l]]) in (row, tail, CSR position) order put into the
    (row, hop, ...) layout: (edges int32 [E, 5], alpha [E], offsets int64 [n + 1], time int32 [E] or None)."""
    counts = torch.stack([torch.bincount(hops[l][0][:, 0].long(), minlength=n) for l in range(1, L + 1)])   # [L, B]
    per_row = counts.sum(0)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=device)
    offsets[1:] = torch.cumsum(per_row, 0)
    n_total = int(offsets[-1].item())
    edges = torch.empty((n_total, 5), dtype=torch.int32, device=device)
    alpha = torch.empty(n_total, dtype=torch.float32, device=device)
    time = torch.empty(n_total, dtype=torch.int32, device=device) if len(hops[1]) > 2 else None
    before = torch.cumsum(counts, 0) - counts          # [L, B]: edges of the row in earlier hops
    for l in range(1, L + 1):
        e, al = hops[l][:2]
        row_first = torch.cumsum(counts[l - 1], 0) - counts[l - 1]
        row_base = offsets[:-1] + before[l - 1]
        engine.explain_gather(l, n, e, al, row_first, row_base, edges, alpha)
        if time is not None:                               # the same placement, as a device index
            r = e[:, 0].long()
            time[row_base[r] + torch.arange(e.shape[0], device=device) - row_first[r]] = hops[l][2]
    return edges, alpha, offsets, time


def explain_temporal(model, batch, objs=None, min_alpha=0.0):
    """T_RED_GNN.explain (see there): the static driver with the temporal hop call; every edge carries its time id."""
    from .temporal import batch_ids, eval_semantics
    device = model.linear_classifier.weight.device
    engine._require_gpu(device)
    heads_h, _, _ = batch_ids(model, batch, "explain")
    n, n_ent = len(heads_h), model.n_ent
    objs_h = None
    if objs is not None:
        objs_h = _ids(objs, "objs")
        if len(objs_h) != n:
            raise ValueError("explain: %d answers for %d rows" % (len(objs_h), n))
        if objs_h.min() < 0 or objs_h.max() >= n_ent:
            raise ValueError("answer id out of range (n_ent=%d)" % n_ent)
    tau = float(min_alpha)
    if tau != tau:
        raise ValueError("explain: min_alpha is NaN")
    L, a = model.n_layer, model.attn_dim
    with torch.no_grad(), eval_semantics(model):
        kept = []
        scores = model._run(batch, "test", kept=kept)
        fr, graph, q_time = kept[0]["frontier"], kept[0]["graph"], kept[0]["q_time"]
        layers = kept[1:]
        if objs_h is None:
            objs_t = scores.argmax(1)                    # first maximum = smallest entity id on a tie
        else:
            objs_t = torch.as_tensor(objs_h, dtype=torch.int64).to(device)
        marks, reached = engine.explain_seed(fr, L, objs_t.to(torch.int32).contiguous())
        zero_b = torch.zeros(1, device=device)           # the temporal attention has no bias
        hops = [None] * (L + 1)
        for l in range(L, 0, -1):
            k = layers[l - 1]
            marks, e, al, tm = engine.texplain_hop(fr, graph, l, marks, k["a_s"].detach().contiguous(), k["a_r"].detach().contiguous(),
                                                   k["a_q"].detach().contiguous(), k["w_alpha"].detach().contiguous(), zero_b, a, tau)
            hops[l] = (e, al, tm)
        if tau > 0.0:
            hops = _forward_sweep(hops, L, n_ent)
        rows = torch.arange(n, device=device)
        score = scores[rows, objs_t].contiguous()
        edges, alpha, offsets, time = _assemble(hops, n, L, device)
    return RDigraph(edges=edges, alpha=alpha, offsets=offsets, reached=reached, score=score, n_hops=L, time=time,
                    q_time=q_time.clone())


def explain_extrapolation(model, X, objs=None, min_alpha=0.0):
    """extrapolation.T_RED_GNN.explain (see there): the temporal driver on the one-graph layout, the hop call testing every edge
    against its query's row window; the third list carried along is the edges' data row."""
    from .extrapolation import _int_ids, check_batch
    from .temporal import eval_semantics
    src, _, _ = check_batch(model, X, "explain")
    n, n_ent = len(src), model.n_ent
    objs_h = None
    if objs is not None:
        objs_h = _int_ids(objs, "explain", "objs")
        if len(objs_h) != n:
            raise ValueError("explain: %d answers for %d rows" % (len(objs_h), n))
        if objs_h.min() < 0 or objs_h.max() >= n_ent:
            raise ValueError("answer id out of range (n_ent=%d)" % n_ent)
    tau = float(min_alpha)
    if tau != tau:
        raise ValueError("explain: min_alpha is NaN")
    device = engine._require_gpu(model.linear_classifier.weight.device)
    L, a = model.n_layer, model.attn_dim
    kept = []
    try:
        with torch.no_grad(), eval_semantics(model):
            logits, _, nodes, _ = model._run(X, dense=False, kept=kept)
            fr, graph, q_time, loop_time = (kept[0][k] for k in ("frontier", "graph", "q_time", "loop_time"))
            layers = kept[1:]
            seg_ptr = torch.searchsorted(nodes[:, 0].contiguous(), torch.arange(n + 1, dtype=torch.int32, device=device))
            ent = nodes[:, 1].contiguous()
            if objs_h is None:                               # each row's own top answer: the smallest id on a tie
                objs_t = engine.segment_topk(logits.contiguous(), ent, seg_ptr, 1, want_prob=False)[0].reshape(-1).long()
            else:
                objs_t = torch.as_tensor(objs_h, dtype=torch.int64).to(device)
            marks, reached = engine.explain_seed(fr, L, objs_t.to(torch.int32).contiguous())
            zero_b = torch.zeros(1, device=device)           # the attention has no bias
            hops = [None] * (L + 1)
            for l in range(L, 0, -1):
                k = layers[l - 1]
                marks, e, al, row = engine.xexplain_hop(fr, graph, l, marks, k["a_s"].detach().contiguous(), k["a_r"].detach().contiguous(),
                                                        k["a_q"].detach().contiguous(), k["w_alpha"].detach().contiguous(), zero_b, a, tau)
                hops[l] = (e, al, row)
            if tau > 0.0:
                hops = _forward_sweep(hops, L, n_ent)
            # the logit of o: its pair's position in the sorted (query, entity) keys
            key = nodes[:, 0].long() * n_ent + nodes[:, 1].long()
            want = torch.arange(n, device=device) * n_ent + objs_t.clamp(min=0)
            pos = torch.searchsorted(key, want).clamp_(max=max(key.numel() - 1, 0))
            score = torch.where(reached & (key[pos] == want), logits[pos], torch.zeros_like(logits[pos])).contiguous()
            edges, alpha, offsets, row = _assemble(hops, n, L, device)
            loop = row >= model.n_data
            time = torch.where(loop, loop_time[edges[:, 0].long()], model.row_time[row.clamp(max=max(model.n_data - 1, 0)).long()])
            data_row = torch.where(loop, torch.full_like(row, -1), row)
    finally:
        if kept:                                             # an exception must not leave a windowed frontier in the pool
            kept[0]["frontier"].set_window(None, None, 0)
    return RDigraph(edges=edges, alpha=alpha, offsets=offsets, reached=reached, score=score, n_hops=L, time=time.to(torch.int32),
                    q_time=q_time.clone(), data_row=data_row)


def _forward_sweep(hops, L, n_ent):
    """Keep the hop-l edges (l >= 2) whose head is the tail of a kept hop-(l-1) edge of the same row: with min_alpha > 0 the backward
    marks alone admit edges whose head is reached from s only through edges below the threshold.  On the compact lists; a temporal
    hop's third list (the edges' times) is carried along."""
    for l in range(2, L + 1):
        prev, e = hops[l - 1][0], hops[l][0]
        reach = torch.unique(prev[:, 0].long() * n_ent + prev[:, 3].long())
        ok = torch.isin(e[:, 0].long() * n_ent + e[:, 1].long(), reach)
        hops[l] = tuple(x[ok].contiguous() for x in hops[l])          # (edges, alpha[, time]): the lists stay aligned
    return hops
