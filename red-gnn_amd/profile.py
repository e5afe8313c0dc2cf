"""Attention profile: when the model answers relation q, which edge relations does it listen to, and at which hop?

    prof = model.attention_profile(subs, rels)            # group="relation": one row per query relation id
    prof.alpha_sum[q, l - 1, rel], prof.count[q, l - 1, rel]
    prof.mean()                                           # mean alpha per cell, NaN where there is no edge
    rel_ids, mean = prof.top(q, k=5)                      # per hop the k edge relations with the largest mean alpha

Over the hop-l edges (b, h, rel, t) of the query subgraphs - exactly the edges the forward aggregates, identity edges included -
count is the number of edges and alpha_sum the sum of their attention, per query (group="query") or per query relation
(group="relation").  Summed over the hops this is the reference's attention_vis table (Temporal/interpolation/model_cuda.py:117-119,
163-166).  The reduction runs in HIP (csrc/profile.hip, rg_attn_profile): one launch per hop re-evaluates alpha with the forward
kernel's arithmetic and adds it as 64-bit fixed point (2^-32 units, per-edge rounding Q = 2^-33), so every cell is an exact integer
sum: bit-identical across runs, across any split of a batch and any order of its queries.  Grouping by relation is an integer
index_add on the device; the conversion to float64 is the last step.

Temporal interpolation (T_RED_GNN.attention_profile, rg_tattn_profile): ``prof = model.attention_profile(batch)`` has one more axis,
the edge's direction against the query time (0 past, 1 now, 2 future): ``prof.count[q, l - 1, dir, rel]``; ``prof.collapse("direction")``
is the three-axis table, ``prof.top(q, k, direction=2)`` ranks the future edges alone.

Temporal extrapolation (extrapolation.T_RED_GNN.attention_profile, rg_xattn_profile): every edge lies in the past, and the third axis is
how far: the edge's lag in days against the query's day, binned by ``lag_edges`` - ``prof.count[q, l - 1, bin, rel]``.
``prof.lag_labels()`` names the bins, ``prof.lag_share(q)`` is the share of each hop's attention mass per bin, ``prof.collapse("lag")``
the three-axis table and ``prof.top(q, k, lag=bin)`` ranks the edges of one bin alone.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import engine

FRACTION_BITS = 32
Q = 2.0 ** -(FRACTION_BITS + 1)          # rounding of one edge's alpha in alpha_sum
DEFAULT_LAG_EDGES = (2, 4, 8, 15, 31, 61, 121)      # days 0-1, 2-3, 4-7, 8-14, 15-30, 31-60, 61-120, 121+
MAX_LAG_EDGES = 255                      # 256 bins: the kernel's bin table is uint8


def check_lag_edges(edges):
    """``edges`` as a tuple of ints: the first day of every lag bin but the first (bin i holds the lags edges[i-1] <= lag < edges[i],
    bin 0 starts at lag 0, the last bin is open-ended).  Strictly ascending non-negative integers, at most 255 of them; () is one
    bin.  ValueError otherwise."""
    try:
        items = list(edges)
    except TypeError:
        raise ValueError("lag_edges must be a sequence of integers (got %r)" % (edges,)) from None
    for e in items:
        if isinstance(e, (bool, np.bool_)) or not isinstance(e, (int, np.integer)):
            raise ValueError("lag_edges must hold integers (got %r)" % (e,))
    out = tuple(int(e) for e in items)
    if len(out) > MAX_LAG_EDGES:
        raise ValueError("lag_edges: at most %d edges (got %d)" % (MAX_LAG_EDGES, len(out)))
    if any(e < 0 for e in out) or any(b <= a for a, b in zip(out, out[1:])):
        raise ValueError("lag_edges must be non-negative and strictly ascending (got %r)" % (out,))
    return out


def lag_bins(lag, edges):
    """The bin of every lag (days): np.searchsorted(edges, lag, side="right")."""
    return np.searchsorted(np.asarray(edges, dtype=np.int64), lag, side="right")


def lag_labels(edges):
    """The lag bins of ``edges`` as (first day, last day) pairs, the last one (first day, None): open-ended.  (A first edge of 0
    leaves bin 0 empty: (0, -1).)"""
    first = (0,) + tuple(edges)
    return [(a, b - 1) for a, b in zip(first, first[1:])] + [(first[-1], None)]


@dataclass
class AttentionProfile:
    """count int64 [G, L, 2R+1] and fixed int64 [G, L, 2R+1] (the sums of alpha in units of 2^-32), on the device that computed them.
    G = 2R+1 query relation ids (group == "relation"; rows of relations not queried are zero) or the B queries in the order given
    (group == "query").  ``axes`` names the dimensions: code that indexes through it keeps working when a setting adds one (the
    temporal models' edge direction).  Profiles of the same grouping add (``+``): integer sums, exact.
    A temporal profile (T_RED_GNN.attention_profile) has axes ("group", "hop", "direction", "relation"), shape [G, L, 3, n_rel+1]:
    direction 0 past / 1 now / 2 future of the edge's time against the query's; ``collapse("direction")`` gives the three-axis table.
    An extrapolation profile (extrapolation.T_RED_GNN.attention_profile) has axes ("group", "hop", "lag", "relation"), shape
    [G, L, len(lag_edges) + 1, n_rel+1], and carries its ``lag_edges`` (see check_lag_edges); profiles of different edges do not add."""
    fixed: torch.Tensor
    count: torch.Tensor
    group: str = "relation"
    axes: tuple = ("group", "hop", "relation")
    lag_edges: tuple = None

    @property
    def alpha_sum(self):
        """float64 [G, L, 2R+1]: the sum of alpha per cell."""
        return self.fixed.double() * 2.0 ** -FRACTION_BITS

    @property
    def n_hops(self):
        return self.count.shape[self.axes.index("hop")]

    def mean(self):
        """float64 [G, L, 2R+1]: mean alpha per cell, NaN where count == 0."""
        c = self.count.double()
        return torch.where(self.count > 0, self.alpha_sum / c.clamp(min=1.0), torch.full_like(c, float("nan")))

    def total(self):
        """The profile summed over the hops, [G, 1, 2R+1]: the reference's attention_vis table."""
        h = self.axes.index("hop")
        return AttentionProfile(self.fixed.sum(h, keepdim=True), self.count.sum(h, keepdim=True), self.group, self.axes, self.lag_edges)

    def collapse(self, axis_name):
        """The profile summed over the named axis (integer sums), which leaves ``axes``: collapse("direction") of a temporal profile
        is the three-axis table of the static models (summed over the hops too: the reference's attention_vis)."""
        if axis_name in ("group", "hop", "relation") or axis_name not in self.axes:
            raise ValueError("collapse: only an axis beyond ('group', 'hop', 'relation') can be summed away, e.g. 'direction' "
                             "(got %r, axes %r); total() sums the hops" % (axis_name, self.axes))
        i = self.axes.index(axis_name)
        return AttentionProfile(self.fixed.sum(i), self.count.sum(i), self.group, self.axes[:i] + self.axes[i + 1:],
                                None if axis_name == "lag" else self.lag_edges)

    def top(self, row, k=5, direction=None, lag=None):
        """Per hop the k edge relations with the largest mean alpha in row ``row`` (a query relation id, or a query's position with
        group == "query"), ties to the smaller relation id.  Returns (relation ids int64 [L, k], mean alpha float64 [L, k]); where
        fewer than k relations have edges the row ends in id -1, mean NaN.  On a profile with a direction axis ``direction`` = 0 / 1 / 2
        selects the edges of one direction and None means all of them (the profile collapsed over direction); without that axis it
        must be None.  ``lag`` does the same on a profile with a lag axis: a bin index, or None for all bins."""
        if "lag" in self.axes:
            if direction is not None:
                raise ValueError("top: this profile has no direction axis (axes %r)" % (self.axes,))
            i, n_bins = self.axes.index("lag"), self.count.shape[self.axes.index("lag")]
            if lag is None:
                return self._top(self.fixed.sum(i), self.count.sum(i), row, k)
            if isinstance(lag, (bool, np.bool_)) or not isinstance(lag, (int, np.integer)) or not 0 <= lag < n_bins:
                raise ValueError("top: lag must be None or a bin index in 0..%d (got %r)" % (n_bins - 1, lag))
            return self._top(self.fixed.select(i, int(lag)), self.count.select(i, int(lag)), row, k)
        if lag is not None:
            raise ValueError("top: this profile has no lag axis (axes %r)" % (self.axes,))
        if "direction" in self.axes:
            if direction is None:
                i = self.axes.index("direction")
                return self._top(self.fixed.sum(i), self.count.sum(i), row, k)
            if isinstance(direction, (bool, np.bool_)) or not isinstance(direction, (int, np.integer)) or not 0 <= direction <= 2:
                raise ValueError("top: direction must be None, 0 (past), 1 (now) or 2 (future) (got %r)" % (direction,))
            i = self.axes.index("direction")
            return self._top(self.fixed.select(i, int(direction)), self.count.select(i, int(direction)), row, k)
        if direction is not None:
            raise ValueError("top: this profile has no direction axis (axes %r)" % (self.axes,))
        return self._top(self.fixed, self.count, row, k)

    @staticmethod
    def _top(fixed, count, row, k):
        """top() on three-axis tables [G, L, relation rows]."""
        n_rows, n_rel_rows = count.shape[0], count.shape[-1]
        if not 0 <= int(row) < n_rows:
            raise ValueError("top: row %d not in 0..%d" % (int(row), n_rows - 1))
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError("top: k must be a positive integer (got %r)" % (k,))
        k = min(int(k), n_rel_rows)
        c = count[int(row)].double()                                              # [L, 2R+1]; the mean as mean() forms it
        mean = torch.where(count[int(row)] > 0, fixed[int(row)].double() * 2.0 ** -FRACTION_BITS / c.clamp(min=1.0),
                           torch.full_like(c, float("nan")))
        key = torch.where(torch.isnan(mean), torch.full_like(mean, -1.0), mean)   # alpha >= 0: cells without edges sort last
        order = torch.argsort(key, dim=-1, descending=True, stable=True)[:, :k]
        best = torch.gather(mean, 1, order)
        ids = torch.where(torch.isnan(best), torch.full_like(order, -1), order)
        return ids, best

    def lag_labels(self):
        """The lag bins as (first day, last day) pairs, the last one (first day, None): open-ended.  (A first edge of 0 leaves bin 0
        empty: (0, -1).)"""
        if "lag" not in self.axes or self.lag_edges is None:
            raise ValueError("lag_labels: this profile has no lag axis (axes %r)" % (self.axes,))
        return lag_labels(self.lag_edges)

    def lag_share(self, row):
        """float64 [L, n_bins]: the share of each hop's attention mass (the sum of alpha over the edge relations) that row ``row`` gives
        to every lag bin; NaN where the hop has no edges."""
        if "lag" not in self.axes:
            raise ValueError("lag_share: this profile has no lag axis (axes %r)" % (self.axes,))
        if self.axes != ("group", "hop", "lag", "relation"):
            raise ValueError("lag_share: axes must be ('group', 'hop', 'lag', 'relation') (got %r)" % (self.axes,))
        if not 0 <= int(row) < self.count.shape[0]:
            raise ValueError("lag_share: row %d not in 0..%d" % (int(row), self.count.shape[0] - 1))
        mass = self.fixed[int(row)].sum(-1).double()                                  # [L, n_bins], integer sums
        whole = mass.sum(-1, keepdim=True)
        has = self.count[int(row)].sum((-1, -2)).unsqueeze(-1) > 0
        return torch.where(has, mass / whole, torch.full_like(mass, float("nan")))

    def __add__(self, other):
        if not isinstance(other, AttentionProfile):
            return NotImplemented
        if other.group != self.group or other.axes != self.axes or other.count.shape != self.count.shape:
            raise ValueError("profiles of different grouping or shape do not add (%s %s, %s %s)"
                             % (self.group, tuple(self.count.shape), other.group, tuple(other.count.shape)))
        if other.lag_edges != self.lag_edges:
            raise ValueError("profiles of different lag edges do not add (%r, %r)" % (self.lag_edges, other.lag_edges))
        return AttentionProfile(self.fixed + other.fixed, self.count + other.count, self.group, self.axes, self.lag_edges)

    def cpu(self):
        return AttentionProfile(self.fixed.cpu(), self.count.cpu(), self.group, self.axes, self.lag_edges)


def _ids(x):
    a = x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return a.astype(np.int64).reshape(-1)


def attention_profile(model, subs, rels, mode="test", group="relation"):
    """RED_GNN_trans.attention_profile (see there)."""
    from .models import _pad4, pad_attn
    device = model.W_final.weight.device
    engine._require_gpu(device)
    if group not in ("relation", "query"):
        raise ValueError("attention_profile: group must be 'relation' or 'query' (got %r)" % (group,))
    subs_h, rels_h = _ids(subs), _ids(rels)
    n = len(subs_h)
    if n == 0 or len(rels_h) != n:
        raise ValueError("attention_profile: need one relation per subject and at least one row (got %d subjects, %d relations)"
                         % (n, len(rels_h)))
    graph = model.loader.graph_for(mode)
    n_ent, n_rows = graph.n_ent, 2 * model.n_rel + 1
    if subs_h.min() < 0 or subs_h.max() >= n_ent or rels_h.min() < 0 or rels_h.max() >= n_rows:
        raise ValueError("query subject / relation id out of range (n_ent=%d, 2*n_rel+1=%d)" % (n_ent, n_rows))
    L = model.n_layer
    d, a = model.hidden_dim, model.attn_dim
    ld, ap = max(16, _pad4(d)), pad_attn(a)
    with torch.no_grad():
        kept = []
        model._run(subs_h, rels_h, mode, kept=kept)
        fr, q_rel = kept[0]["frontier"], kept[0]["q_rel"]
        layers = kept[1:]
        tables = [k["tables"] for k in layers]
        if any(t is None for t in tables):
            tables = model.inference_tables(q_rel, ld, ap)
        fixed = torch.zeros((L, n, n_rows), dtype=torch.int64, device=device)
        count = torch.zeros((L, n, n_rows), dtype=torch.int64, device=device)
        for l in range(1, L + 1):
            layer = model.gnn_layers[l - 1]
            a_r, a_q, _ = tables[l - 1]
            engine.attn_profile(fr, graph, l, layers[l - 1]["a_s"].detach().contiguous(), a_r.contiguous(), a_q.contiguous(),
                                layer.w_alpha.weight.detach().reshape(-1).contiguous(), layer.w_alpha.bias.detach().contiguous(), a,
                                fixed[l - 1], count[l - 1])
        fixed, count = fixed.transpose(0, 1), count.transpose(0, 1)               # [B, L, 2R+1]
        if group == "relation":                                                  # integer adds: exact whatever their order
            fixed = torch.zeros((n_rows, L, n_rows), dtype=torch.int64, device=device).index_add_(0, q_rel, fixed)
            count = torch.zeros((n_rows, L, n_rows), dtype=torch.int64, device=device).index_add_(0, q_rel, count)
    return AttentionProfile(fixed=fixed.contiguous(), count=count.contiguous(), group=group)


def attention_profile_temporal(model, batch, group="relation"):
    """T_RED_GNN.attention_profile (see there)."""
    from .temporal import batch_ids, eval_semantics
    device = model.linear_classifier.weight.device
    engine._require_gpu(device)
    if group not in ("relation", "query"):
        raise ValueError("attention_profile: group must be 'relation' or 'query' (got %r)" % (group,))
    heads_h, _, _ = batch_ids(model, batch, "attention_profile")
    n, L, a, n_rows = len(heads_h), model.n_layer, model.attn_dim, model.n_rel + 1
    with torch.no_grad(), eval_semantics(model):
        kept = []
        model._run(batch, "test", kept=kept)
        fr, graph, q_rel, q_time = kept[0]["frontier"], kept[0]["graph"], kept[0]["q_rel"], kept[0]["q_time"]
        layers = kept[1:]
        zero_b = torch.zeros(1, device=device)           # the temporal attention has no bias
        fixed = torch.zeros((L, n, 3, n_rows), dtype=torch.int64, device=device)
        count = torch.zeros((L, n, 3, n_rows), dtype=torch.int64, device=device)
        for l in range(1, L + 1):
            k = layers[l - 1]
            engine.tattn_profile(fr, graph, l, q_time.contiguous(), k["a_s"].detach().contiguous(), k["a_r"].detach().contiguous(),
                                 k["a_q"].detach().contiguous(), k["w_alpha"].detach().contiguous(), zero_b, a, fixed[l - 1], count[l - 1])
        fixed, count = fixed.transpose(0, 1), count.transpose(0, 1)               # [B, L, 3, n_rel+1]
        if group == "relation":                                                  # integer adds: exact whatever their order
            fixed = torch.zeros((n_rows, L, 3, n_rows), dtype=torch.int64, device=device).index_add_(0, q_rel, fixed)
            count = torch.zeros((n_rows, L, 3, n_rows), dtype=torch.int64, device=device).index_add_(0, q_rel, count)
    return AttentionProfile(fixed=fixed.contiguous(), count=count.contiguous(), group=group,
                            axes=("group", "hop", "direction", "relation"))


def attention_profile_extrapolation(model, X, group="relation", lag_edges=DEFAULT_LAG_EDGES):
    """extrapolation.T_RED_GNN.attention_profile (see there)."""
    from .extrapolation import check_batch
    from .temporal import eval_semantics
    if group not in ("relation", "query"):
        raise ValueError("attention_profile: group must be 'relation' or 'query' (got %r)" % (group,))
    edges = check_lag_edges(lag_edges)
    src, _, _ = check_batch(model, X, "attention_profile")
    device = engine._require_gpu(model.linear_classifier.weight.device)
    n, L, a, n_rows, n_bins = len(src), model.n_layer, model.attn_dim, model.n_rel + 1, len(edges) + 1
    kept = []
    try:
        with torch.no_grad(), eval_semantics(model):
            model._run(X, dense=False, kept=kept)
            fr, graph, q_rel, q_time, loop_time = (kept[0][k] for k in ("frontier", "graph", "q_rel", "q_time", "loop_time"))
            layers = kept[1:]
            # one entry per row of the forward's time table: the kernel clamps an edge's lag exactly as the forward clamps its row
            lag_bin = torch.as_tensor(lag_bins(np.arange(kept[0]["n_tab"]), edges).astype(np.uint8)).to(device)
            zero_b = torch.zeros(1, device=device)           # the attention has no bias
            fixed = torch.zeros((L, n, n_bins, n_rows), dtype=torch.int64, device=device)
            count = torch.zeros((L, n, n_bins, n_rows), dtype=torch.int64, device=device)
            for l in range(1, L + 1):
                k = layers[l - 1]
                engine.xattn_profile(fr, graph, l, q_time.contiguous(), loop_time.contiguous(), model.row_time, lag_bin, n_bins,
                                     k["a_s"].detach().contiguous(), k["a_r"].detach().contiguous(), k["a_q"].detach().contiguous(),
                                     k["w_alpha"].detach().contiguous(), zero_b, a, fixed[l - 1], count[l - 1])
            fixed, count = fixed.transpose(0, 1), count.transpose(0, 1)               # [B, L, n_bins, n_rel+1]
            if group == "relation":                                                  # integer adds: exact whatever their order
                fixed = torch.zeros((n_rows, L, n_bins, n_rows), dtype=torch.int64, device=device).index_add_(0, q_rel, fixed)
                count = torch.zeros((n_rows, L, n_bins, n_rows), dtype=torch.int64, device=device).index_add_(0, q_rel, count)
    finally:
        if kept:                                             # an exception must not leave a windowed frontier in the pool
            kept[0]["frontier"].set_window(None, None, 0)
    return AttentionProfile(fixed=fixed.contiguous(), count=count.contiguous(), group=group,
                            axes=("group", "hop", "lag", "relation"), lag_edges=edges)


def split_profile(model, loader, data="test", batch=50, max_queries=None):
    """The group="relation" profile of the queries of the valid or test split (BaseModel.attention_profile): batches of ``batch``
    queries, their integer tables added."""
    if data not in ("valid", "test"):
        raise ValueError("attention_profile: data must be 'valid' or 'test' (got %r)" % (data,))
    query = loader.valid_q if data == "valid" else loader.test_q
    n = len(query) if max_queries is None else min(len(query), int(max_queries))
    if n <= 0 or batch <= 0:
        raise ValueError("attention_profile: no queries to profile in the %s split (n=%d, batch=%d)" % (data, n, batch))
    mode = loader.eval_mode(data) if hasattr(loader, "eval_mode") else data
    subs, rels = np.array([q[0] for q in query[:n]]), np.array([q[1] for q in query[:n]])
    prof = None
    for lo in range(0, n, batch):
        part = model.attention_profile(subs[lo:lo + batch], rels[lo:lo + batch], mode=mode, group="relation")
        prof = part if prof is None else prof + part
    return prof
