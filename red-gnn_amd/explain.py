"""The relational digraph (r-digraph) behind an answer, with its attention weights.

For a query (s, r) and an answer o, RED-GNN's score of o depends only on the edges of the union of all length-L relational paths
s -> o through the query's subgraph (identity self-loops count as steps); each edge carries its layer's attention alpha.

    rd = model.explain(subs, rels, objs)            # objs=None: the model's own top answer per row
    rd.edges[rd.offsets[b]:rd.offsets[b + 1]]       # (row, hop, head, rel, tail) of row b, hop 1..L
    rels_, ents, prod = rd.strongest_paths()         # the path of largest alpha product per row
    paths = rd.top_paths(k=4)                        # the k best paths per row (HIP: csrc/paths.hip), an explain.PathSet
    table = model.rules(subs, rels, objs, k=2)       # their relation sequences counted as rules: an explain.RuleTable
    rs = rd.rescore(model, keep=~paths.fact_mask(1))  # o re-scored with the best path's facts deleted (HIP: csrc/digraph_fwd.hip)
    fid = model.fidelity(subs, rels, objs, k=4)      # necessity and sufficiency of the best 1..k paths: an explain.Fidelity
    sal = rd.saliency(model)                         # d score / d (a gate on every edge), one pass (HIP: csrc/digraph_bwd.hip): an explain.Saliency
    att = rd.integrated_gradients(model, steps=16)   # attributions that add up to the score (gated, replicated edge-list kernels): an explain.Attribution
    mask = rd.learn_mask(model)                      # the small set of facts that reproduces the score (a gate per replica and edge, csrc/mask_step.hip): an explain.EdgeMask
    mask = rd.learn_tied_mask(model, tie="fact")     # ... with one gate per fact, per (hop, relation) or per caller label (csrc/mask_tie.hip)

The extraction runs in HIP (csrc/explain.hip): a forward keeps all L + 1 frontier levels and each layer's attention projection, then
one backward marking pass per hop reads only the marked tails' CSR rows.  This module holds the result type and the host drivers.

Temporal interpolation (T_RED_GNN.explain, rg_texplain_*): ``rd = model.explain(batch, objs)`` with the batch dict of forward; every
edge also carries its time id (``rd.time``), ``rd.q_time`` is the rows' query time and ``rd.direction()`` the forward's past / now /
future of each edge.  ``rd.rescore(model, keep)`` re-scores the answers on the kept edges (rg_digraph_tlayer_fwd), ``rd.fact_mask``
takes quadruples (h, r, t, time id) and ``model.fidelity(batch, objs, k, inverse_offset)`` is the static model's fidelity;
``rd.saliency(model)`` / ``model.saliency(batch, objs)`` is its edge saliency (rg_digraph_tlayer_bwd on directed source rows), facts
being quadruples there.  ``table = model.rules(batch, objs, k=2)`` counts the best paths as temporal rules, steps (relation, direction)
with identity steps written as direction 3 = any (TemporalRuleTable), and ``model.rule_quality(table)`` counts how they hold in the
quadruple graph per anchor (entity, query time id) (TemporalRuleQuality; engine.trule_ground, csrc/trule_ground.hip).

Temporal extrapolation (extrapolation.T_RED_GNN.explain, rg_xexplain_*): ``rd = model.explain(X, objs)`` with the batch object of
forward; ``rd.data_row`` names the past fact behind every edge (-1: a self-loop, relation id n_rel), ``rd.time`` its day and
``rd.lag()`` how many days before the query it lies.  ``table = model.rules(X, objs, k=2)`` counts the best paths as lag-binned rules,
steps (relation, lag bin) under the ``lag_edges`` of attention_profile with identity steps written as ANY (LagRuleTable), and
``model.rule_quality(table)`` counts how they hold in the model's own data per anchor (entity, query day) under the forward's row
windows (LagRuleQuality; engine.xrule_ground, csrc/xrule_ground.hip); ``model.rule_scores(quality, X)`` / ``rule_predict`` /
``rule_evaluate`` apply the weighted rules to queries (engine.xrule_apply, csrc/xrule_apply.hip).  ``rd.rescore(model, keep)`` re-scores
the forecasts on the kept edges with the windows as they were - per hop the index of the live edges built in HIP from the hop's own
edges (engine.digraph_hop_index, csrc/digraph_index.hip) and one rg_digraph_tlayer_fwd launch in its n_dir = 1 form -, ``rd.fact_mask``
takes (s, p, o, day), ``rd.data_row_mask`` data rows, and ``model.fidelity(X, objs, k, inverse_offset)`` / ``fidelity_all`` are the static
model's fidelity; ``rd.saliency(model)`` / ``model.saliency(X, objs)`` is its edge saliency (rg_digraph_tlayer_bwd, n_dir = 1), with
``Saliency.data_row_grad()`` per data row.
"""
import types
from dataclasses import dataclass, fields, replace

import numpy as np
import torch
import torch.nn.functional as F

from . import engine
from .models import _pad4, pad_attn
from .profile import FRACTION_BITS                       # sums in units of 2^-32, as the attention profile's
from .profile import DEFAULT_LAG_EDGES, check_lag_edges, lag_labels


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
    q_sub    int64 [B]     the subject s of each row
    q_rel    int64 [B]     ... and its query relation r; ``rescore`` needs both
    n_rel    int           static and inductive: the KG's relation count (ids >= n_rel are inverses, 2 * n_rel the identity);
                           temporal interpolation: the model's n_rel, the identity's relation id (the tables have n_rel + 1 rows);
                           extrapolation: the model's n_rel_true, the identity's relation id; ``fact_mask`` needs it
    n_time   int           temporal interpolation only (None otherwise): the number of time ids; with it ``rescore`` and ``fact_mask``
                           take the digraph as a temporal interpolation one, with ``data_row`` and without it as an extrapolation one
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
    q_sub: torch.Tensor = None
    q_rel: torch.Tensor = None
    n_rel: int = None
    n_time: int = None

    def rescore(self, model, keep=None, mode="test", gate=None):
        """The model's score of o on the digraph with only the edges ``keep`` (bool or uint8 [E] over ``edges``; None: all of them):
        an explain.Rescore.  RED-GNN's score of o depends on the r-digraph's edges alone, so this is the model's score on the knowledge
        graph with the facts behind the dropped edges deleted - a forward over the compact edge list, one HIP message-passing launch
        per hop (rg_digraph_layer_fwd; csrc/digraph_fwd.hip) and the dense step of the inference forward, no graph rebuild.  A kept
        edge whose head is no longer visited one hop down is dead (``live``); a row whose o has no length-L walk left scores exactly 0.
        ``model``: the RED_GNN_trans / RED_GNN_induc that explained, ``mode`` the one it explained in.  Eval semantics under no_grad.
        A temporal interpolation digraph (temporal.T_RED_GNN.explain: ``time``, ``q_time``, ``q_sub``, ``q_rel``, ``n_rel`` and
        ``n_time`` set) is re-scored by the temporal.T_RED_GNN that explained it, one rg_digraph_tlayer_fwd launch per hop with the
        tables T_RED_GNN's forward forms; ``mode`` must be "test" there, the full graph explain walks.  The digraph is checked on the
        host first (ValueError); any mix of temporal fields and models is a ValueError.

        An extrapolation digraph (extrapolation.T_RED_GNN.explain: ``data_row``, ``time``, ``q_time``, ``q_sub``, ``q_rel`` and
        ``n_rel`` set, ``n_time`` None) is re-scored by the extrapolation.T_RED_GNN that explained it, ``mode`` "test": the inference
        branch of its forward over the kept edges, per hop the index built in HIP from the hop's own edges (rg_digraph_hop_index,
        csrc/digraph_index.hip; the digraph is validated there, on the device) and one rg_digraph_tlayer_fwd launch in its n_dir = 1
        form.  No frontier, no window and no [B, n_ent] array: ``time`` already holds the day the forward used for every edge, a
        self-loop's first window day included.  What it answers is "the forward with these edges absent AND THE WINDOWS AS THEY
        WERE".  The reference's time_offset_list makes a window start at the last row of day begin - 1 and end before the last row
        of day cur_t - 1, with offset 0 for days without rows, so deleting rows from the data itself moves window boundaries when a
        deleted row is the last of its day or a day loses all its rows; the rescore equals the forward of a model rebuilt from the
        reduced data only for deletions that do neither.

        ``gate`` float32 [E] (a tensor or a numpy array, every entry finite; None: the ungated path, unchanged): the soft-gated rescore of
        a static digraph - gate[e] multiplies the message of the kept edge e, agg[o] = sum_e gate_e alpha_e (hidden[s] + rela[r]), in
        rg_digraph_layer_fwd_gated.  ``live`` and ``reached`` stay structural: they follow ``keep`` alone, and a gate of 0 disconnects
        nothing.  A gate of ones gives the ungated call's bits.  The timed forms of the gated kernels are not built: a temporal or
        extrapolation digraph or model with a gate is a ValueError."""
        return rescore(self, model, keep, mode, gate)

    def saliency(self, model, keep=None, mode="test", gate=None):
        """How much the score of o depends on every edge: an explain.Saliency.  Give every edge e a gate g_e that multiplies its
        message, agg[o] = sum_e g_e alpha_e (hidden[s] + rela[r]) in the forward ``rescore`` states; ``edge_grad[e]`` is d score / d g_e
        at g == 1 with the parameters fixed.  The gate does not enter alpha_e directly; it does enter the attention of later hops
        through the states.  One pass instead of one ``rescore`` per fact: the hop loop of ``rescore`` (same checks, same ``keep``,
        the same ``score``, ``reached``, ``live`` and ``alpha`` bit for bit), then the hops backwards - the dense step's adjoint
        through tall_linear / gru_step with the parameters detached, the edge-list layer's in HIP (rg_digraph_layer_bwd,
        csrc/digraph_bwd.hip: no float atomics, the same bits on every run).  Dead edges and rows whose answer is not reached get
        exactly 0.

        The driver follows the model's class.  A static or inductive model walks a static digraph as above (a temporal or
        extrapolation digraph is a ValueError there).  A temporal.T_RED_GNN walks the temporal interpolation digraph it explained
        and an extrapolation.T_RED_GNN its extrapolation digraph: ``rescore``'s hop loop for that family, then per hop the
        activation's adjoint, the timed edge-list layer's in HIP (rg_digraph_tlayer_bwd: a directed source row per work item) and
        plain products with the direction linears and the attention projection - neither model has a GRU or a carry.  The message
        gated there is the directed one, hidden_dir + (rela_dir + time row); ``mode`` must be "test".  A digraph of another
        family than the model's is a ValueError.

        ``gate`` float32 [E] (as ``rescore``'s; static digraphs only): ``edge_grad`` is the gradient at that gate instead of at 1, the
        score, alpha and the states being those of ``rescore(gate=gate)`` (rg_digraph_layer_fwd_gated / rg_digraph_layer_bwd_gated).  A
        gate of ones gives the ungated call's bits."""
        return saliency(self, model, keep, mode, gate)

    def integrated_gradients(self, model, steps=16, keep=None, baseline=None, target=None, rep_chunk=None, mode="test"):
        """An attribution that adds up: integrated gradients of the score of o along the straight path of gates from ``baseline`` to
        ``target``, an explain.Attribution.  edge_attr[e] = (target_e - baseline_e) * the mean over the path of d score / d g_e, so by
        the fundamental theorem of calculus a row's edge_attr sum to score(target) - score(baseline); the quadrature is the midpoint
        rule, t_k = (k + 1/2) / steps with weights 1 / steps, and ``residual`` is what it leaves.  ``baseline`` None: the identity edges
        (relation 2 * n_rel) at 1 and every other edge at 0 - self-loops are part of the model, not facts; ``target`` None: 1
        everywhere; both can be given as float32 [E].  ``keep`` as in ``rescore``.

        The per-hop index and the source views are built once; the steps then run as REPLICAS of the hop in one launch per hop
        (rg_digraph_layer_fwd_gated, rg_digraph_layer_bwd_gated), their rows stacked for the dense step and its autograd adjoint, in
        groups of ``rep_chunk`` steps.  ``rep_chunk`` None: as many as keep replicas * edges at or under explain.IG_REP_EDGES = 2^20,
        which bounds the stacked states at 2^20 rows per hop.  The sums run over k ascending, so the result does not depend on the run;
        it depends on ``rep_chunk`` in the last bits only (the dense products see other row counts).  Static and inductive models; a
        temporal or extrapolation digraph or model is a ValueError: the timed forms of the gated kernels are not built."""
        return integrated_gradients(self, model, steps, keep, baseline, target, rep_chunk, mode)

    def learn_mask(self, model, lambdas=(0.01, 0.03, 0.1, 0.3, 1.0), entropy=0.0, iterations=100, lr=0.05, theta0=2.0, tol=0.05, keep=None,
                   mode="test"):
        """Which small set of facts reproduces this answer's score?  A learned edge mask (the GNNExplainer question asked of an
        r-digraph): an explain.EdgeMask.  Every FREE edge - kept and no self-loop; the self-loops (relation 2 * n_rel) are part of the
        model and stay at gate 1, edges not kept are outside the walk - gets a logit theta, starting at ``theta0``, and the gate
        g = sigmoid(theta) that multiplies its message as in ``rescore(gate=)``.  With target the row's score at gate 1, baseline_score
        its score with the free edges at 0 and scale = |target - baseline_score|, Adam (``lr``; beta 0.9 / 0.999, eps 1e-8) minimises
        per row

            ((score(g) - target) / scale)^2  +  lambda * mean of the row's free gates  +  entropy * sum of their binary entropies

        for every lambda of ``lambdas`` at once: the lambdas are REPLICAS of the walk with a gate per (replica, edge), one launch per
        hop for all of them (rg_digraph_layer_fwd_gates, rg_digraph_layer_bwd_gates), and the whole update - chain rule,
        regularisers, Adam, the new gates and their per-row sums - is one more launch per iteration (rg_mask_step,
        csrc/mask_step.hip).  The per-hop index and the source views are built once.  The dense step's autograd adjoint runs per
        replica (explain.MASK_SPLIT_DENSE), so that R replicas in one call give, bit for bit, the gates of R one-replica calls: the
        library GEMMs behind it round by row count, the HIP kernels do not.  A row with scale == 0 or whose answer is not
        reached has no score term (its 1 / scale is taken as 0): its mask only decays under lambda and entropy.

        After ``iterations`` steps (0: the initial gates) every replica's gates are rounded at 0.5 and scored in one stacked gated
        forward (``hard_score``: the other edges at gate 0, which is not deletion - the attention of the edges that stay is what it was);
        a row takes the replica with the fewest gates above 0.5 among those with |hard_score - target| <= ``tol`` * scale, or, if there
        is none, the replica of the smallest deviation, ties to the lower replica.  ``keep`` / ``gate`` of the result are assembled from
        the rows' replicas and ``kept_score`` is one exact ``rescore(keep=)`` of that mask: the facts really deleted.  ``keep`` (the
        argument) as in ``rescore``.  The defaults are a starting point, not a tuned setting.  No float atomics anywhere: the same bits
        on every run.  Static and inductive models; a temporal or extrapolation digraph or model is a ValueError: the timed forms of
        the gated kernels are not built.  A gate per FACT, per (hop, relation) or per label instead of per edge: ``learn_tied_mask``."""
        return learn_mask(self, model, lambdas, entropy, iterations, lr, theta0, tol, keep, mode)

    def learn_tied_mask(self, model, tie="fact", **kw):
        """``learn_mask`` with TIED gates: one logit per group of free edges, every member edge reading the group's gate - an
        explain.EdgeMask whose ``group*`` fields are set.  ``learn_mask`` learns a gate per edge, and a fact usually has several edges
        in a row's digraph (the same fact at two hops, and its inverse): untied, the copies get different gates, ``keep`` can hold one
        copy and drop another - a state the graph can never be in - and ``size`` counts edges.  ``tie`` (explain.mask_groups):

            "fact"      a group per base fact (h, r, t) of a row, inverses folded back - ``fact_mask``'s rule.  The mask is a set of
                        facts: ``keep`` is a ``fact_mask`` of the selected facts (and the kept self-loops), ``size`` counts facts
            "relation"  a group per (hop, relation) of a row: a soft rule body, "which relations, at which hop, carry this answer"
                        (``EdgeMask.format_groups``), next to model.rules
            int64 [E]   any labels >= 0 on the free edges (entity, relation alone, ...): a group per (row, label)

        ``**kw``: ``learn_mask``'s arguments, with the same meaning; the size penalty is lambda * the mean of the row's GROUP gates and
        the entropy term runs over groups.  The state is [R, G]; an iteration is ``learn_mask``'s stacked walk at the [R, E] gates,
        then the chain rule through the tie - d score / d gate_group = the sum over the group's edges of d score / d gate_edge, in
        chunks of 32 members in a fixed order (rg_mask_tie_grad, csrc/mask_tie.hip) -, rg_mask_step on the group arrays and the group
        gates copied to the edges (rg_mask_tie_gates).  No float atomics: the same bits on every run, and a replica's are those of a
        one-replica call.  Where every group is one edge the group gradients are the edges', bit for bit; the gates are
        ``learn_mask``'s up to rg_mask_step's own rounding, which follows a cell's position in its row.  ``size``, ``replica_size`` and
        ``history.size`` / ``history.count`` count groups; ``n_free`` still counts edges.  ``tie`` is checked with ``learn_mask``'s
        own arguments (ValueError "learn_mask: tie ..."), a label tensor's dtype and shape after the digraph's tensors.
        explain.learn_mask(rd, model, ..., tie=) is the same call."""
        return learn_mask(self, model, tie=tie, **kw)

    def fact_mask(self, facts, rows=None, inverse_offset=None):
        """bool [E]: the edges that stand for one of the facts ``facts`` int [F, 3] = (h, r, t), at any hop: an edge is marked if its
        (head, rel, tail) is a fact or a fact's twin (t, inv(r), h), inv(r) = r + n_rel below n_rel and r - n_rel from there on.  The
        identity relation 2 * n_rel is never marked: a self-loop is part of the model, not a fact.  ``rows`` int [F]: fact f counts
        for the edges of row rows[f] only (None: for every row).  Static digraphs that carry ``n_rel``.

        On a temporal interpolation digraph ``facts`` is int [F, 4] = (h, r, t, time id): an edge is marked if its (head, rel, tail,
        time) is one of them - every copy of a quadruple the graph holds more than once - and never the identity relation ``n_rel``.
        How a quadruple graph writes inverses belongs to the data, not to the model: with ``inverse_offset`` = m the twin
        (t, r + m if r < m else r - m, h, time id) is marked too (None: the quadruples as given).  A static digraph takes no
        ``inverse_offset``.

        On an extrapolation digraph ``facts`` is int [F, 4] = (s, p, o, day), days not negative: every data-row edge whose (head,
        rel, tail, ``time``) is one of them is marked - every copy of a row the data hold more than once - and with
        ``inverse_offset`` = m (2 m <= n_rel) the twin (o, p + m or p - m, s, day) too; a self-loop is never marked.
        ``data_row_mask`` names a fact by its exact identity, the data row."""
        return fact_mask(self, facts, rows, inverse_offset)

    def data_row_mask(self, data_rows, rows=None):
        """bool [E]: the edges whose ``data_row`` is one of ``data_rows`` int [F] (not negative; a self-loop has none).  ``rows`` int
        [F]: entry f counts for the edges of row rows[f] only.  Extrapolation digraphs only: there the data row is the exact
        identity of a fact."""
        return data_row_mask(self, data_rows, rows)

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

    def top_paths(self, k=1, scratch_bytes=engine.PATHS_SCRATCH_BYTES):
        """Per row the k best length-L paths s -> o inside the digraph, as a PathSet: by alpha product (float64, left to right, as
        strongest_paths forms it), then by the smaller (head, rel, edge index) of the last edge, then by the order of the prefixes one
        level down.  k = 1 is strongest_paths' path.  One HIP launch per chunk of rows (rg_paths_topk; csrc/paths.hip) on the compact
        edge list: no graph and no model, so static, inductive, temporal and min_alpha-pruned digraphs all work.  ``scratch_bytes``
        bounds the kernel's tables; the rows are walked in chunks that fit (one row at least) and the result does not depend on it.
        The digraph is checked on the host first (ValueError); it must live on the device."""
        if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= k <= engine.PATHS_MAX_K:
            raise ValueError("top_paths: k must be an integer in 1..%d (got %r)" % (engine.PATHS_MAX_K, k))
        if isinstance(scratch_bytes, (bool, np.bool_)) or not isinstance(scratch_bytes, (int, np.integer)) or scratch_bytes < 0:
            raise ValueError("top_paths: scratch_bytes must be a non-negative integer (got %r)" % (scratch_bytes,))
        if isinstance(self.n_hops, (bool, np.bool_)) or not isinstance(self.n_hops, (int, np.integer)) or not 1 <= self.n_hops <= 32:
            raise ValueError("top_paths: n_hops must be an integer in 1..32 (got %r)" % (self.n_hops,))
        e, a, o = self.edges, self.alpha, self.offsets
        if not all(torch.is_tensor(t) for t in (e, a, o)):
            raise ValueError("top_paths: edges, alpha and offsets must be tensors")
        if e.dtype != torch.int32 or e.dim() != 2 or e.shape[1] != 5:
            raise ValueError("top_paths: edges must be int32 [E, 5] (got %s %s)" % (e.dtype, tuple(e.shape)))
        if a.dtype != torch.float32 or a.shape != (e.shape[0],):
            raise ValueError("top_paths: alpha must be float32 [%d] (got %s %s)" % (e.shape[0], a.dtype, tuple(a.shape)))
        if o.dtype != torch.int64 or o.dim() != 1 or o.numel() < 1:
            raise ValueError("top_paths: offsets must be int64 [B + 1] (got %s %s)" % (o.dtype, tuple(o.shape)))
        off = o.detach().cpu().numpy()
        if off[0] != 0 or off[-1] != e.shape[0] or (np.diff(off) < 0).any():
            raise ValueError("top_paths: offsets must start at 0, never decrease and end at the number of edges (%d)" % e.shape[0])
        if not (e.is_cuda and a.is_cuda and o.is_cuda):
            raise ValueError("top_paths: the selection runs in HIP and needs the digraph on the device (got CPU tensors); "
                             "strongest_paths() works on the host")
        edge, product, count = engine.paths_topk(e.contiguous(), a.contiguous(), o.contiguous(), int(self.n_hops), int(k),
                                                 int(scratch_bytes), offsets_host=off)
        return PathSet(edge=edge, product=product, count=count, digraph=self)


@dataclass
class PathSet:
    """The k best paths of every row of an r-digraph (RDigraph.top_paths), best first.  Tensors on the digraph's device.

    edge     int64 [B, k, L]  indices into digraph.edges, hop 1..L; -1 where the row has fewer than k paths
    product  float64 [B, k]   the paths' alpha products; 0 where absent
    count    int32 [B]        paths found for the row (<= k)
    digraph  RDigraph         the digraph the indices point into
    """
    edge: torch.Tensor
    product: torch.Tensor
    count: torch.Tensor
    digraph: RDigraph

    def _gather(self, column, absent):
        """column [E] read through ``edge``; ``absent`` where there is no path."""
        if column.shape[0] == 0:
            return torch.full(self.edge.shape, absent, dtype=column.dtype, device=self.edge.device)
        got = column[self.edge.clamp(min=0)]
        return torch.where(self.edge >= 0, got, torch.full_like(got, absent))

    def rels(self):
        """int64 [B, k, L]: the relation of every step, -1 where absent."""
        return self._gather(self.digraph.edges[:, 3].long(), -1)

    def entities(self):
        """int64 [B, k, L+1]: the entities from s to o, -1 where absent."""
        e = self.digraph.edges
        return torch.cat([self._gather(e[:, 2].long(), -1), self._gather(e[:, 4].long(), -1)[..., -1:]], -1)

    def alphas(self):
        """float32 [B, k, L]: the attention of every step, 0 where absent."""
        return self._gather(self.digraph.alpha, 0.0)

    def times(self):
        """int32 [B, k, L]: the time id of every step, -1 where absent.  Temporal digraphs only."""
        if self.digraph.time is None:
            raise ValueError("times: a static r-digraph has no edge times")
        return self._gather(self.digraph.time, -1)

    def data_rows(self):
        """int32 [B, k, L]: the data row of the fact behind every step (-1: a self-loop, or absent).  Extrapolation digraphs only."""
        if self.digraph.data_row is None:
            raise ValueError("data_rows: this r-digraph carries no data rows (extrapolation digraphs do)")
        return self._gather(self.digraph.data_row, -1)

    def fact_mask(self, j, inverse_offset=None):
        """bool [E]: digraph.fact_mask of the facts the best ``j`` paths of each row step over (1 <= j <= k; a row with fewer paths
        gives all it has), every fact for its own row.  Identity steps are no facts.  On a temporal digraph the facts are the steps'
        quadruples and ``inverse_offset`` is passed on."""
        k = self.edge.shape[1]
        _check_count(j, "fact_mask", "j", k)
        rd = self.digraph
        at = self.edge[:, :int(j)].reshape(-1)
        at = at[at >= 0]
        e = rd.edges[at].long()
        if _has_times(rd):
            _check_temporal_fields(rd, "fact_mask")
            return rd.fact_mask(torch.cat([e[:, 2:5], rd.time[at].long()[:, None]], 1), rows=e[:, 0], inverse_offset=inverse_offset)
        return rd.fact_mask(e[:, 2:5], rows=e[:, 0], inverse_offset=inverse_offset)


def _check_count(x, who, name, most=None):
    """``x`` is an integer >= 1 (and <= ``most``), or ValueError."""
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)) or x < 1 or (most is not None and x > most):
        want = "a positive integer" if most is None else "an integer in 1..%d" % most
        raise ValueError("%s: %s must be %s (got %r)" % (who, name, want, x))


def _cpu(x):
    """A dataclass with every tensor of it, and every table in it, on the host."""
    return replace(x, **{f.name: getattr(x, f.name).cpu() for f in fields(x) if hasattr(getattr(x, f.name), "cpu")})


class _Rules:
    """What the three rule tables share: a subclass is a dataclass with the tensors head [R], support [R], fixed [R] and body [R, L]
    among its fields, rows sorted by its key, and the int n_rel."""

    cpu = _cpu

    def product_sum(self):
        """float64 [R]: the sum of the alpha products of each rule's paths."""
        return self.fixed.double() * 2.0 ** -FRACTION_BITS

    def mean(self):
        """float64 [R]: the mean alpha product of each rule's paths."""
        return self.product_sum() / self.support.double()

    def _rows(self, rows):
        return replace(self, **{f.name: getattr(self, f.name)[rows] for f in fields(self) if torch.is_tensor(getattr(self, f.name))})

    def top(self, q_rel, n):
        """The n rules of query relation ``q_rel`` with the largest support (ties: the smaller body, or key), as a table in that order."""
        _check_count(n, "top", "n")
        rows = torch.nonzero(self.head == int(q_rel)).reshape(-1)                 # ascending: key order
        return self._rows(rows[torch.argsort(-self.support[rows], stable=True)][:int(n)])

    def _check_add(self, other):
        if other.n_rel != self.n_rel or other.body.shape[1] != self.body.shape[1]:
            raise ValueError("rule tables of different relation count or path length do not add (n_rel %d / %d, L %d / %d)"
                             % (self.n_rel, other.n_rel, self.body.shape[1], other.body.shape[1]))


@dataclass
class RuleTable(_Rules):
    """Paths counted as rules: one row per distinct (query relation, relation sequence r_1..r_L), sorted by (head, body).

    head     int64 [R]      the query relation
    body     int64 [R, L]   the relations of the steps (the identity id 2 * n_rel kept as is)
    support  int64 [R]      paths counted
    fixed    int64 [R]      the sum of their alpha products in units of 2^-32, each path rounded once: tables add exactly
    n_rel    int            the KG's relation count (ids >= n_rel are inverses, 2 * n_rel the identity)
    """
    head: torch.Tensor
    body: torch.Tensor
    support: torch.Tensor
    fixed: torch.Tensor
    n_rel: int

    def __add__(self, other):
        if not isinstance(other, RuleTable):
            return NotImplemented
        self._check_add(other)
        key = torch.cat([torch.cat([self.head[:, None], self.body], 1), torch.cat([other.head[:, None], other.body], 1)], 0)
        return _table(key, torch.cat([self.support, other.support]), torch.cat([self.fixed, other.fixed]), self.n_rel)

    def format(self, id2rel=None):
        """One string per rule, ``r1(x,z1) ^ r2^-1(z1,y) -> q(x,y)``: identity steps dropped, ids >= n_rel printed as inverses of
        id - n_rel; ``id2rel`` names the relations (a sequence or dict), else r<id>."""
        def name(r):
            if r == 2 * self.n_rel:
                return "id"
            base = r - self.n_rel if r >= self.n_rel else r
            label = str(id2rel[base]) if id2rel is not None else "r%d" % base
            return label + ("^-1" if r >= self.n_rel else "")
        out = []
        for h, b in zip(self.head.tolist(), self.body.tolist()):
            steps = [r for r in b if r != 2 * self.n_rel]
            var = ["x"] + ["z%d" % i for i in range(1, len(steps))] + ["y"]
            lhs = " ^ ".join("%s(%s,%s)" % (name(r), var[i], var[i + 1]) for i, r in enumerate(steps)) if steps else "x=y"
            out.append("%s -> %s(x,y)" % (lhs, name(h)))
        return out


class _StepRules(_Rules):
    """What TemporalRuleTable and LagRuleTable share: a step is a relation and a second id, held in the field ``_step`` names
    ("direction", "lag_bin"); the fields are head, body, that one, support, fixed and then what does not change with the rows."""

    def key(self):
        """int64 [R, 1 + 2L]: (head, r_1, s_1, .., r_L, s_L), s the direction or lag bin of the step: the key the rows are sorted by."""
        R, L = self.body.shape
        return torch.cat([self.head[:, None], torch.stack([self.body, getattr(self, self._step)], 2).reshape(R, 2 * L)], 1)

    @classmethod
    def _merged(cls, key, support, fixed, *rest):
        """The table of rows key int64 [P, 1 + 2L] = (head, r_1, s_1, .., r_L, s_L), equal keys merged: _table on the wide key.
        ``rest``: the fields after ``fixed``, n_rel last."""
        t = _table(key, support, fixed, rest[-1])
        return cls(t.head, t.body[:, 0::2].contiguous(), t.body[:, 1::2].contiguous(), t.support, t.fixed, *rest)

    def __add__(self, other):
        if not isinstance(other, type(self)):
            return NotImplemented
        self._check_add(other)
        return self._merged(torch.cat([self.key(), other.key()], 0), torch.cat([self.support, other.support]),
                            torch.cat([self.fixed, other.fixed]), *(getattr(self, f.name) for f in fields(self)[5:]))

    def _format(self, id2rel, tag):
        """One string per rule, ``r3<tag>(x,z1) ^ r1<tag>(z1,y) -> r0(x,y)``, ``tag(s)`` the text after a step's relation; identity
        steps dropped, the head without a tag."""
        name = lambda r: str(id2rel[r]) if id2rel is not None else "r%d" % r
        out = []
        for h, b, d in zip(self.head.tolist(), self.body.tolist(), getattr(self, self._step).tolist()):
            steps = [(r, k) for r, k in zip(b, d) if r != self.n_rel]
            var = ["x"] + ["z%d" % i for i in range(1, len(steps))] + ["y"]
            lhs = " ^ ".join("%s%s(%s,%s)" % (name(r), tag(k), var[i], var[i + 1]) for i, (r, k) in enumerate(steps)) if steps else "x=y"
            out.append("%s -> %s(x,y)" % (lhs, name(h)))
        return out


@dataclass
class _Quality:
    """What RuleQuality, TemporalRuleQuality and LagRuleQuality share: the rules and their four counts, the ratios of the counts and
    the ordering of ``top``.  A subclass adds its last field (n_sources, n_anchors) and the methods trivial() and _tie_key()."""
    table: _Rules
    body_pairs: torch.Tensor
    hits: torch.Tensor
    pca_body_pairs: torch.Tensor
    head_pairs: torch.Tensor

    cpu = _cpu

    def _ratio(self, den):
        num, den = self.hits.double(), den.double()
        return torch.where(den > 0, num / den.clamp(min=1.0), torch.zeros_like(num))

    def confidence(self):
        """float64 [R]: hits / body_pairs (standard confidence), 0.0 where the body connects nothing."""
        return self._ratio(self.body_pairs)

    def pca_confidence(self):
        """float64 [R]: hits / pca_body_pairs (confidence under the partial-completeness assumption), 0.0 where that is 0."""
        return self._ratio(self.pca_body_pairs)

    def head_coverage(self):
        """float64 [R]: hits / head_pairs, 0.0 where the head relation has no fact from a source."""
        return self._ratio(self.head_pairs)

    def top(self, q_rel, n, by="confidence", min_hits=1, drop_trivial=True):
        """Row indices (int64, at most n) of the best rules of query relation ``q_rel`` by "confidence", "pca_confidence" or "hits",
        among those with hits >= min_hits (and not trivial).  Ties go to the larger hits, then to the smaller body."""
        _check_count(n, "top", "n")
        if by not in ("confidence", "pca_confidence", "hits"):
            raise ValueError("top: by must be 'confidence', 'pca_confidence' or 'hits' (got %r)" % (by,))
        q = self.cpu()                                   # a few thousand rows at most: ordered on the host
        score = (q.hits.double() if by == "hits" else getattr(q, by)()).numpy()
        hits, body = q.hits.numpy(), q._tie_key().numpy()
        keep = (q.table.head == int(q_rel)) & (q.hits >= int(min_hits))
        if drop_trivial:
            keep = keep & ~q.trivial()
        rows = np.nonzero(keep.numpy())[0]
        keys = [body[rows, c] for c in reversed(range(body.shape[1]))] + [-hits[rows], -score[rows]]     # lexsort: last key first
        rows = rows[np.lexsort(keys)][:int(n)] if rows.size else rows
        return torch.as_tensor(rows, dtype=torch.int64).to(self.hits.device)

    def format(self, id2rel=None):
        """table.format() with ``hits/body_pairs conf=... pca=...`` appended to every line."""
        q = self.cpu()
        conf, pca = q.confidence().tolist(), q.pca_confidence().tolist()
        return ["%s  %d/%d conf=%.4f pca=%.4f" % (line, h, b, c, p)
                for line, h, b, c, p in zip(q.table.format(id2rel), q.hits.tolist(), q.body_pairs.tolist(), conf, pca)]


@dataclass
class RuleQuality(_Quality):
    """How the rules of a RuleTable hold in a knowledge graph (engine.rule_ground; csrc/rule_ground.hip): exact counts over the pairs
    (x, y) with x one of ``n_sources`` source entities, on the graph as built (inverse and identity rows included, a repeated fact
    counted once).  body(x, y): the rule's relation sequence leads from x to y, identity steps being ordinary steps.

    table           RuleTable  the rules, row by row
    body_pairs      int64 [R]  pairs the body connects
    hits            int64 [R]  ... that the head relation connects too (AMIE's support; ``table.support`` counts explained paths)
    pca_body_pairs  int64 [R]  pairs the body connects whose x has some fact of the head relation
    head_pairs      int64 [R]  pairs the head relation connects
    n_sources       int        number of source entities

    hits <= pca_body_pairs <= body_pairs and hits <= head_pairs.  confidence(), pca_confidence(), head_coverage(), top() and format()
    and cpu() are _Quality's, and so are the first five fields.
    """
    n_sources: int

    def trivial(self):
        """bool [R]: the body with its identity steps dropped is exactly [head]; such a rule has confidence 1 by construction."""
        step = self.table.body != 2 * self.table.n_rel
        return (step.sum(1) == 1) & ((self.table.body * step).sum(1) == self.table.head)

    def _tie_key(self):
        return self.table.body


DIRECTION_ANY = 3                                        # a step that matches every edge time (engine.TRULE_DIRECTIONS)


@dataclass
class TemporalRuleTable(_StepRules):
    """Paths of the temporal interpolation model counted as rules: one row per distinct (query relation, (r_1, d_1), .., (r_L, d_L)),
    sorted by that key.  d is the direction of the step's edge against the query time as the forward forms it (RDigraph.direction():
    0 past, 1 now, 2 future); an identity step (relation id n_rel; the reference gives those rows the sentinel time n_time - 1) is
    written with direction 3 = any, so a rule does not split by where its padding fell.

    head       int64 [R]      the query relation
    body       int64 [R, L]   the relations of the steps
    direction  int64 [R, L]   their directions, 0..3
    support    int64 [R]      paths counted
    fixed      int64 [R]      the sum of their alpha products in units of 2^-32, each path rounded once: tables add exactly
    n_rel      int            the model's n_rel: relation ids 0..n_rel-1 as the quadruples hold them, n_rel the identity
    """
    head: torch.Tensor
    body: torch.Tensor
    direction: torch.Tensor
    support: torch.Tensor
    fixed: torch.Tensor
    n_rel: int
    _step = "direction"

    def format(self, id2rel=None):
        """One string per rule, ``r3[past](x,z1) ^ r1(z1,y) -> r0(x,y)``: every step with its direction in brackets (none for
        "any"), identity steps dropped, the head - a "now" fact - without a tag; ``id2rel`` names the relation ids (a sequence or
        dict), else r<id>."""
        return self._format(id2rel, lambda k: "" if k == DIRECTION_ANY else "[%s]" % engine.TRULE_DIRECTIONS[k])


@dataclass
class TemporalRuleQuality(_Quality):
    """How the rules of a TemporalRuleTable hold in the quadruple graph (engine.trule_ground; csrc/trule_ground.hip): exact counts over
    the pairs ((x, t), y) with (x, t) one of ``n_anchors`` anchors - an entity and a query time id - on the graph as built, a repeated
    row counted once.  body(x, y | t): the steps lead from x to y through rows whose time stands to t as each step's direction says;
    head(x, y | t): the graph has the row (x, head, y, t).

    table           TemporalRuleTable  the rules, row by row
    body_pairs      int64 [R]  pairs the body connects
    hits            int64 [R]  ... that are facts of the head relation at the anchor's time too
    pca_body_pairs  int64 [R]  pairs the body connects whose anchor has some fact of the head relation at its time
    head_pairs      int64 [R]  pairs the head relation connects at the anchors' times
    n_anchors       int        number of anchors

    hits <= pca_body_pairs <= body_pairs and hits <= head_pairs.  confidence(), pca_confidence(), head_coverage(), top() and format()
    and cpu() are _Quality's, and so are the first five fields.
    """
    n_anchors: int

    def trivial(self):
        """bool [R]: the body with its identity steps dropped is exactly [(head, now)]; such a rule has confidence 1 by construction."""
        t = self.table
        step = t.body != t.n_rel
        return (step.sum(1) == 1) & ((t.body * step).sum(1) == t.head) & ((t.direction * step).sum(1) == 1)

    def _tie_key(self):
        return self.table.key()[:, 1:]


@dataclass
class LagRuleTable(_StepRules):
    """Paths of the extrapolation model counted as rules: one row per distinct (query relation, (r_1, b_1), .., (r_L, b_L)), sorted
    by that key.  Every edge of the forecasting model lies in the past, so a step is told apart by how far back its fact lies: b is the
    bin of the edge's lag in days (RDigraph.lag(): query day minus the edge's day) under ``lag_edges``, the bins of profile.lag_bins
    and of attention_profile; bin len(lag_edges) + 1 is ANY.  An identity step (relation id n_rel) is always written as ANY, so a rule
    does not split by where its padding fell.

    head       int64 [R]      the query relation
    body       int64 [R, L]   the relations of the steps
    lag_bin    int64 [R, L]   their lag bins, 0..len(lag_edges) + 1
    support    int64 [R]      paths counted
    fixed      int64 [R]      the sum of their alpha products in units of 2^-32, each path rounded once: tables add exactly
    lag_edges  tuple          the first day of every lag bin but the first (profile.check_lag_edges)
    n_rel      int            the identity's relation id: the model's n_rel_true (extrapolation.T_RED_GNN.n_rel is one more)
    """
    head: torch.Tensor
    body: torch.Tensor
    lag_bin: torch.Tensor
    support: torch.Tensor
    fixed: torch.Tensor
    lag_edges: tuple
    n_rel: int
    _step = "lag_bin"

    def __post_init__(self):
        self.lag_edges = check_lag_edges(self.lag_edges)

    @property
    def any_bin(self):
        """The bin id that stands for any lag: len(lag_edges) + 1."""
        return len(self.lag_edges) + 1

    def _check_add(self, other):
        if other.n_rel != self.n_rel or other.body.shape[1] != self.body.shape[1] or other.lag_edges != self.lag_edges:
            raise ValueError("rule tables of different relation count, path length or lag edges do not add (n_rel %d / %d, L %d / %d, "
                             "lag_edges %r / %r)" % (self.n_rel, other.n_rel, self.body.shape[1], other.body.shape[1], self.lag_edges,
                                                     other.lag_edges))

    def lag_ranges(self):
        """(lag_lo, lag_hi) int64 [R, L]: the days [lag_lo, lag_hi) of every step's bin, as engine.xrule_ground takes them.  The
        last bin's hi and ANY's hi are 2^31 - 1; ANY starts at 0."""
        first = torch.tensor((0,) + self.lag_edges + (0,), dtype=torch.int64, device=self.lag_bin.device)
        last = torch.tensor(self.lag_edges + (engine.XRULE_ANY_HI, engine.XRULE_ANY_HI), dtype=torch.int64, device=self.lag_bin.device)
        return first[self.lag_bin], last[self.lag_bin]

    def format(self, id2rel=None):
        """One string per rule, ``r3[2-3d](x,z1) ^ r7[61-120d](z1,y) -> r1(x,y)``: every step with the days of its lag bin in
        brackets, as AttentionProfile.lag_labels() names them (``[121+d]`` for the open last bin, none for ANY), identity steps
        dropped, the head - a fact of the query day - without a tag; ``id2rel`` names the relation ids (a sequence or dict), else
        r<id>."""
        labels = ["[%d+d]" % a if b is None else ("[%dd]" % a if a == b else "[%d-%dd]" % (a, b)) for a, b in lag_labels(self.lag_edges)]
        labels.append("")
        return self._format(id2rel, labels.__getitem__)


@dataclass
class LagRuleQuality(_Quality):
    """How the rules of a LagRuleTable hold in the forecasting model's own data (engine.xrule_ground; csrc/xrule_ground.hip): exact
    counts over the pairs ((x, t), y) with (x, t) one of ``n_anchors`` anchors - an entity and a query day - a repeated row counted
    once.  body(x, y | t): the steps lead from x to y through rows of day t's window whose lag lies in each step's bin; head(x, y | t):
    the data hold a row (x, head, y) of day t itself.

    table           LagRuleTable  the rules, row by row
    body_pairs      int64 [R]  pairs the body connects
    hits            int64 [R]  ... that are facts of the head relation on the anchor's day too
    pca_body_pairs  int64 [R]  pairs the body connects whose anchor has some fact of the head relation on its day
    head_pairs      int64 [R]  pairs the head relation connects on the anchors' days
    n_anchors       int        number of anchors

    hits <= pca_body_pairs <= body_pairs and hits <= head_pairs.  confidence(), pca_confidence(), head_coverage(), top() and format()
    and cpu() are _Quality's, and so are the first five fields.
    """
    n_anchors: int

    def trivial(self):
        """bool [R]: all False - no window holds a fact of the query day, so no body restates its head."""
        return torch.zeros(self.hits.shape[0], dtype=torch.bool, device=self.hits.device)

    def _tie_key(self):
        return self.table.key()[:, 1:]


def rule_quality(model, table, mode="test", sources=None, scratch_bytes=engine.RULE_SCRATCH_BYTES):
    """RED_GNN_trans.rule_quality (see there)."""
    if not isinstance(table, RuleTable):
        raise ValueError("rule_quality: table must be an explain.RuleTable (got %s)" % type(table).__name__)
    if table.n_rel != model.n_rel:
        raise ValueError("rule_quality: the table has n_rel=%d, the model n_rel=%d" % (table.n_rel, model.n_rel))
    graph = model.loader.graph_for(mode)
    counts = engine.rule_ground(graph, table.head, table.body, sources, scratch_bytes)
    n_sources = graph.n_ent if sources is None else int(len(sources))
    return RuleQuality(table, *(counts[:, c].contiguous() for c in range(4)), n_sources)


def split_rule_quality(base, table=None, data="test", k=1, max_queries=None):
    """BaseModel.rule_quality: the table (default: base.rules(data, k, max_queries)) counted on the graph split_rows picks for
    ``data``."""
    if data not in ("valid", "test"):
        raise ValueError("rule_quality: data must be 'valid' or 'test' (got %r)" % (data,))
    if table is None:
        table = base.rules(data, k, max_queries)
    mode = base.loader.eval_mode(data) if hasattr(base.loader, "eval_mode") else data
    return base.model.rule_quality(table, mode=mode)


AGGREGATIONS = ("noisy_or", "max")


def _check_agg(agg, who):
    if agg not in AGGREGATIONS:
        raise ValueError("%s: agg must be 'noisy_or' or 'max' (got %r)" % (who, agg))


@dataclass
class RuleScores:
    """What the rules of a RuleQuality predict for a batch of queries (s, r, ?) (engine.rule_apply; csrc/rule_apply.hip), per (query,
    entity) cell over the rules kept.  A rule fires for (b, y) iff its head is the query relation and its body leads from s to y in
    the graph; the rules that fire are folded in table order.  Tensors on the device that computed them, [B, n_ent] each.

    best       float32  the largest weight among the rules that fire (0 where none does)
    surv       float32  the product of their (1 - weight), each factor and each product rounded to float32, in table order
    best_rule  int32    the table row of the first rule with weight ``best`` (-1 where none fires)
    fired      int32    how many rules fire
    rows       int64 [K] the table rows of the rules kept, ascending (the weights were formed for these)
    """
    best: torch.Tensor
    surv: torch.Tensor
    best_rule: torch.Tensor
    fired: torch.Tensor
    rows: torch.Tensor

    def score(self, agg="noisy_or"):
        """float32 [B, n_ent]: 'noisy_or' = fl32(1 - surv), 'max' = best (AnyBURL's max aggregation); 0 where no rule fires."""
        _check_agg(agg, "score")
        return self.best if agg == "max" else 1.0 - self.surv

    def covered(self):
        """bool [B, n_ent]: some rule reaches the entity."""
        return self.fired > 0


@dataclass
class RulePrediction:
    """The k best answers of each query by rule score.  ids int64 [B, k] (-1 past the row's remaining entities), scores float32 [B, k]
    (-inf past the end), rule int64 [B, k] the table row of the answer's best rule (-1: no rule reaches it, or past the end), fired
    int32 [B, k] how many rules reach it (0 past the end).  An answer with score 0 and fired 0 is one no rule reaches: it is listed
    only because fewer than k entities are reached.  ``table``: the RuleTable the rows refer to."""
    ids: torch.Tensor
    scores: torch.Tensor
    rule: torch.Tensor
    fired: torch.Tensor
    table: RuleTable = None

    def format(self, id2rel=None):
        """One line per answer, B * k in row order: ``row b #j: entity <id> score <s> fired <n>  <the best rule as RuleTable.format>``;
        ``-`` for the rule where none fires."""
        lines = self.table.cpu().format(id2rel) if self.table is not None else None
        ids, sc, rule, fired = (t.cpu().tolist() for t in (self.ids, self.scores, self.rule, self.fired))
        out = []
        for b in range(len(ids)):
            for j in range(len(ids[b])):
                r = rule[b][j]
                text = "-" if r < 0 else (lines[r] if lines is not None else "rule %d" % r)
                out.append("row %d #%d: entity %d score %.6f fired %d  %s" % (b, j, ids[b][j], sc[b][j], fired[b][j], text))
        return out


def rule_weights(quality, by="confidence", laplace=0.0, min_hits=1, drop_trivial=True):
    """(rows int64 [K], weight float32 [K]) on the host: the rules of ``quality`` kept for scoring, in table order, and their weights
    float32(hits / (den + laplace)) formed in float64, den = body_pairs (by="confidence") or pca_body_pairs ("pca_confidence").  Kept:
    hits >= min_hits, weight > 0, and not trivial() unless ``drop_trivial`` is False.  ``quality``: a RuleQuality, a
    TemporalRuleQuality or a LagRuleQuality (the same counts and trivial(), which is all False for the last; the drivers check which
    of the three they take)."""
    if not isinstance(quality, (RuleQuality, TemporalRuleQuality, LagRuleQuality)):
        raise ValueError("rule_scores: quality must be an explain.RuleQuality (got %s)" % type(quality).__name__)
    if by not in ("confidence", "pca_confidence"):
        raise ValueError("rule_scores: by must be 'confidence' or 'pca_confidence' (got %r)" % (by,))
    laplace = float(laplace)
    if not (np.isfinite(laplace) and laplace >= 0.0):
        raise ValueError("rule_scores: laplace must be a finite number >= 0 (got %r)" % (laplace,))
    q = quality.cpu()
    hits = q.hits.numpy().astype(np.float64)
    den = (q.body_pairs if by == "confidence" else q.pca_body_pairs).numpy().astype(np.float64) + laplace
    weight = np.where(den > 0, hits / np.where(den > 0, den, 1.0), 0.0).astype(np.float32)
    keep = (q.hits.numpy() >= int(min_hits)) & (weight > 0)
    if drop_trivial:
        keep &= ~q.trivial().numpy()
    rows = np.nonzero(keep)[0].astype(np.int64)
    return rows, weight[rows]


def _rule_scores(best, surv, best_rule, fired, rows):
    """RuleScores of the four outputs of engine.rule_apply / trule_apply on the rules ``rows`` of a table (int64 on the host):
    best_rule goes from kept-rule index to table row."""
    rows_d = torch.as_tensor(rows).to(best.device)
    if rows_d.numel():
        best_rule = torch.where(best_rule >= 0, rows_d.int()[best_rule.clamp(min=0).long()], best_rule)
    return RuleScores(best, surv, best_rule, fired, rows_d)


def _rule_prediction(rs, k, agg, q_key, known, table):
    """RulePrediction of the k best entities of every row of the RuleScores ``rs`` under ``agg`` (engine.topk with its filter
    ``q_key``, ``known``), each with its best rule and how many fired; empty tensors for a batch without rows."""
    device = rs.best.device
    if rs.best.shape[0] == 0:
        z = lambda dt, fill: torch.full((0, int(k)), fill, dtype=dt, device=device)
        return RulePrediction(z(torch.int64, -1), z(torch.float32, 0.0), z(torch.int64, -1), z(torch.int32, 0), table)
    idx, val = engine.topk(rs.score(agg).contiguous(), int(k), q_key, known)
    ids = idx.long()
    at = ids.clamp(min=0)
    rule = torch.where(ids >= 0, rs.best_rule.gather(1, at).long(), torch.full_like(ids, -1))
    fired = torch.where(ids >= 0, rs.fired.gather(1, at), torch.zeros_like(idx))
    return RulePrediction(ids, val, rule, fired, table)


def rule_scores(model, quality, subs, rels, by="confidence", laplace=0.0, min_hits=1, drop_trivial=True, mode="test",
                scratch_bytes=engine.RULE_SCRATCH_BYTES):
    """RED_GNN_trans.rule_scores (see there)."""
    if not isinstance(quality, RuleQuality):
        raise ValueError("rule_scores: quality must be an explain.RuleQuality (got %s)" % type(quality).__name__)
    rows, weight = rule_weights(quality, by, laplace, min_hits, drop_trivial)
    table = quality.table
    if table.n_rel != model.n_rel:
        raise ValueError("rule_scores: the table has n_rel=%d, the model n_rel=%d" % (table.n_rel, model.n_rel))
    graph = model.loader.graph_for(mode)
    head, body = table.head.cpu().numpy()[rows], table.body.cpu().numpy()[rows]
    best, surv, best_rule, fired = engine.rule_apply(graph, head, body, weight, _ids(subs, "subs"), _ids(rels, "rels"), scratch_bytes)
    return _rule_scores(best, surv, best_rule, fired, rows)


def rule_predict(model, quality, subs, rels, k=10, agg="noisy_or", exclude_known=True, mode="test", **kw):
    """RED_GNN_trans.rule_predict (see there)."""
    from .prediction import K_MAX, _known_on_device
    _check_agg(agg, "rule_predict")
    _check_count(k, "rule_predict", "k", K_MAX)
    subs_h, rels_h = _ids(subs, "subs"), _ids(rels, "rels")
    rs = rule_scores(model, quality, subs_h, rels_h, mode=mode, **kw)
    device = rs.best.device
    known, q_key = None, None
    if exclude_known:
        known = _known_on_device(model.loader, mode, device)
        q_key = torch.as_tensor(subs_h * (2 * model.n_rel + 1) + rels_h, dtype=torch.int64).to(device)
    return _rule_prediction(rs, k, agg, q_key, known, quality.table)


def split_rule_ranks(base, quality, data="test", agg="noisy_or", batch=256, max_queries=None, **kw):
    """(ranks float64 [n] on the device in (query, ascending answer) order, number of answers some rule reaches) of the rule scores
    over the first ``max_queries`` queries of a split, walked in batches of ``batch`` queries: the body of BaseModel.rule_evaluate."""
    from .utils import cal_ranks_csr
    if data not in ("valid", "test"):
        raise ValueError("rule_evaluate: data must be 'valid' or 'test' (got %r)" % (data,))
    _check_agg(agg, "rule_evaluate")
    _check_count(batch, "rule_evaluate", "batch")
    loader = base.loader
    n_all = len(loader.valid_q if data == "valid" else loader.test_q)
    n = n_all if max_queries is None else min(n_all, int(max_queries))
    if n <= 0:
        raise ValueError("rule_evaluate: no queries in the %s split (n=%d)" % (data, n))
    mode = loader.eval_mode(data) if hasattr(loader, "eval_mode") else data
    ranks, covered = [], 0
    for lo in range(0, n, int(batch)):
        idx = np.arange(lo, min(lo + int(batch), n))
        subs, rels, ans_ptr, ans_idx, filt_ptr, filt_idx = loader.get_batch_csr(idx, data=data)
        rs = base.model.rule_scores(quality, subs, rels, mode=mode, **kw)
        ranks.append(cal_ranks_csr(rs.score(agg), ans_ptr, ans_idx, filt_ptr, filt_idx))
        q_of = torch.repeat_interleave(torch.arange(len(idx), device=ans_ptr.device), (ans_ptr[1:] - ans_ptr[:-1]).long())
        covered += int((rs.fired[q_of, ans_idx.long()] > 0).sum())
    return torch.cat(ranks).double(), covered


def split_rule_evaluate(base, quality=None, data="test", mine="valid", k=1, agg="noisy_or", batch=256, max_queries=None, **kw):
    """BaseModel.rule_evaluate (see there)."""
    from .utils import cal_performance
    if data not in ("valid", "test"):
        raise ValueError("rule_evaluate: data must be 'valid' or 'test' (got %r)" % (data,))
    if mine not in ("valid", "test"):
        raise ValueError("rule_evaluate: mine must be 'valid' or 'test' (got %r)" % (mine,))
    _check_agg(agg, "rule_evaluate")
    if quality is None:
        quality = base.rule_quality(data=mine, k=k, max_queries=max_queries)
    ranks, covered = split_rule_ranks(base, quality, data, agg, batch, max_queries, **kw)
    mrr, h1, h10 = cal_performance(ranks.cpu().numpy())
    n = int(ranks.numel())
    return dict(mrr=float(mrr), h1=float(h1), h10=float(h10), n=n, coverage=covered / n)


def _temporal_quality(model, quality, who):
    if not isinstance(quality, TemporalRuleQuality):
        raise ValueError("%s: quality must be an explain.TemporalRuleQuality (got %s)" % (who, type(quality).__name__))
    if quality.table.n_rel != model.n_rel:
        raise ValueError("%s: the table has n_rel=%d, the model n_rel=%d" % (who, quality.table.n_rel, model.n_rel))


def _temporal_queries(model, batch, who):
    """temporal.batch_ids, and three empty arrays for a batch without rows (rule_scores and rule_predict take one)."""
    from .temporal import batch_ids
    if all(k in batch and len(batch[k]) == 0 for k in ("head", "relation", "time")):
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    return batch_ids(model, batch, who)


def temporal_rule_scores(model, quality, batch, by="confidence", laplace=0.0, min_hits=1, drop_trivial=True,
                         scratch_bytes=engine.RULE_SCRATCH_BYTES, who="rule_scores"):
    """T_RED_GNN.rule_scores (see there)."""
    _temporal_quality(model, quality, who)
    rows, weight = rule_weights(quality, by, laplace, min_hits, drop_trivial)
    heads, rels, times = _temporal_queries(model, batch, who)
    t = quality.table
    head, body, direction = (x.cpu().numpy()[rows] for x in (t.head, t.body, t.direction))
    best, surv, best_rule, fired = engine.trule_apply(model.graph, head, body, direction, weight, heads, rels, times, scratch_bytes)
    return _rule_scores(best, surv, best_rule, fired, rows)


def temporal_rule_predict(model, quality, batch, k=10, agg="noisy_or", known=None, **kw):
    """T_RED_GNN.rule_predict (see there)."""
    from .prediction import K_MAX
    _check_agg(agg, "rule_predict")
    _check_count(k, "rule_predict", "k", K_MAX)
    if known is not None and (not isinstance(known, (tuple, list)) or len(known) != 3):
        raise ValueError("rule_predict: known must be the (keys, ptr, idx) triple of temporal_known_index")
    rs = temporal_rule_scores(model, quality, batch, who="rule_predict", **kw)
    heads, rels, times = _temporal_queries(model, batch, "rule_predict")
    device = rs.best.device
    q_key = None
    if known is not None and rs.best.shape[0]:
        known = tuple(torch.as_tensor(x).to(device=device, dtype=dt).contiguous()
                      for x, dt in zip(known, (torch.int64, torch.int64, torch.int32)))
        q_key = torch.as_tensor((heads * (model.n_rel + 1) + rels) * model.n_time + times, dtype=torch.int64).to(device)
    return _rule_prediction(rs, k, agg, q_key, known, quality.table)


def temporal_filter_lists(keys_of, tails, known):
    """(ptr int32 [B + 1], idx int32) of the filter sets rg_rank takes: per query the sorted union of its tail and the tails the index
    ``known`` = (keys, ptr, idx) numpy arrays (None: nothing) lists for its key.  A set that contains the answer."""
    lists = []
    for key, tail in zip(keys_of.tolist(), tails.tolist()):
        mine = [tail]
        if known is not None:
            at = int(np.searchsorted(known[0], key))
            if at < len(known[0]) and known[0][at] == key:
                mine = np.union1d(known[2][known[1][at]:known[1][at + 1]], mine)
        lists.append(np.asarray(mine, np.int32))
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    return ptr, np.concatenate(lists).astype(np.int32)


def _rule_metrics(ranks, covered, n):
    """The dict temporal_rule_evaluate and lag_rule_evaluate return: n, coverage = covered / n and hits1 / hits3 / hits10 / mrr / mr
    of ``ranks`` = {suffix: list of float64 rank tensors, n ranks in all} for every suffix of evaluation.KINDS; sums in float64."""
    out = {"n": n, "coverage": covered / n}
    for sfx, parts in ranks.items():
        rank = torch.cat(parts).cpu().numpy()
        out["hits1" + sfx], out["hits3" + sfx], out["hits10" + sfx] = (float(np.sum(rank <= c) / n) for c in (1, 3, 10))
        out["mrr" + sfx], out["mr" + sfx] = float(np.sum(1.0 / rank) / n), float(np.sum(rank) / n)
    return out


def temporal_rule_evaluate(model, quads, quality=None, mine=None, k=1, agg="noisy_or", known=None, known_static=None, batch_size=256,
                           **kw):
    """T_RED_GNN.rule_evaluate (see there)."""
    from .evaluation import KINDS, _check_known, check_quads
    from .utils import cal_ranks_csr
    who = "rule_evaluate"
    _check_agg(agg, who)
    if (quality is None) == (mine is None):
        raise ValueError("%s: give exactly one of quality (a TemporalRuleQuality) and mine (quadruples to mine the rules from)" % who)
    _check_count(k, who, "k", engine.PATHS_MAX_K)
    q = check_quads(model, quads, batch_size, who)
    _check_known(known, who, "known")
    _check_known(known_static, who, "known_static")
    if quality is None:
        quality = model.rule_quality(model.rules_all(check_quads(model, mine, 1, who + " (mine)"), k))
    _temporal_quality(model, quality, who)
    host = lambda kn: None if kn is None else tuple(np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x) for x in kn)
    known, known_static = host(known), host(known_static)
    device = model.linear_classifier.weight.device
    to = lambda a: torch.as_tensor(a).to(device)
    ranks, covered = {sfx: [] for sfx in KINDS.values()}, 0
    for lo in range(0, len(q), int(batch_size)):
        b = q[lo:lo + int(batch_size)]
        rs = temporal_rule_scores(model, quality, {"head": b[:, 0], "relation": b[:, 1], "time": b[:, 3]}, who=who, **kw)
        score = rs.score(agg).contiguous()
        tails = to(b[:, 2].astype(np.int32))
        ans_ptr = torch.arange(len(b) + 1, dtype=torch.int32, device=device)
        key_hr = b[:, 0] * (model.n_rel + 1) + b[:, 1]
        for sfx, keys_of, index in (("", key_hr, None), ("_fil_t", key_hr * model.n_time + b[:, 3], known), ("_fil", key_hr, known_static)):
            filt_ptr, filt_idx = temporal_filter_lists(keys_of, b[:, 2], index)
            ranks[sfx].append(cal_ranks_csr(score, ans_ptr, tails, to(filt_ptr), to(filt_idx)).double())
        covered += int((rs.fired.gather(1, tails.long()[:, None]) > 0).sum())
    return _rule_metrics(ranks, covered, len(q))


def _lag_quality(model, quality, who):
    if not isinstance(quality, LagRuleQuality):
        raise ValueError("%s: quality must be an explain.LagRuleQuality (got %s)" % (who, type(quality).__name__))
    if quality.table.n_rel != model.n_rel_true:
        raise ValueError("%s: the table has n_rel=%d, the model n_rel=%d" % (who, quality.table.n_rel, model.n_rel_true))


def _lag_queries(model, X, who):
    """extrapolation.check_batch, and three empty arrays for a batch without rows (rule_scores and rule_predict take one)."""
    from .extrapolation import check_batch
    if all(len(x) == 0 for x in (X.src_idx, X.rel_idx, X.ts)):
        z = np.zeros(0, np.int64)
        return z, z.copy(), z.copy()
    return check_batch(model, X, who)


def lag_rule_scores(model, quality, X, by="confidence", laplace=0.0, min_hits=1, scratch_bytes=engine.RULE_SCRATCH_BYTES,
                    who="rule_scores"):
    """extrapolation.T_RED_GNN.rule_scores (see there)."""
    from .extrapolation import WINDOW
    _lag_quality(model, quality, who)
    rows, weight = rule_weights(quality, by, laplace, min_hits)          # (no rule of this family is trivial)
    src, rel, ts = _lag_queries(model, X, who)
    t = quality.table
    head, body, lag_lo, lag_hi = (x.cpu().numpy()[rows] for x in (t.head, t.body) + tuple(t.lag_ranges()))
    win_lo, win_hi = model.windows()
    best, surv, best_rule, fired = engine.xrule_apply(model.graph, head, body, lag_lo, lag_hi, weight, src, rel, ts // model.time_granularity,
                                                      model._row_time_host, win_lo, win_hi, WINDOW, scratch_bytes)
    return _rule_scores(best, surv, best_rule, fired, rows)


def lag_rule_predict(model, quality, X, k=10, agg="noisy_or", known=None, **kw):
    """extrapolation.T_RED_GNN.rule_predict (see there)."""
    from .extrapolation import KnownObjects
    from .prediction import K_MAX
    _check_agg(agg, "rule_predict")
    _check_count(k, "rule_predict", "k", K_MAX)
    if known is not None and not isinstance(known, KnownObjects):
        raise ValueError("rule_predict: known must be a KnownObjects index (extrapolation.known_objects_index)")
    rs = lag_rule_scores(model, quality, X, who="rule_predict", **kw)
    src, rel, ts = _lag_queries(model, X, "rule_predict")
    device = rs.best.device
    q_key = known_dev = None
    if known is not None and rs.best.shape[0]:
        q_key = torch.as_tensor(known.query_keys(src, rel, ts)).to(device)
        known_dev = model._index_on_device(known, device)
    return _rule_prediction(rs, k, agg, q_key, known_dev, quality.table)


def anchors_before(anchors, day, who="rule_evaluate"):
    """The rows of ``anchors`` int [S, 2] = (entity, day) whose day is below ``day``; ValueError where none is."""
    a = np.asarray(anchors, np.int64).reshape(-1, 2)
    a = a[a[:, 1] < int(day)]
    if len(a) == 0:
        raise ValueError("%s: no anchor lies before the earliest query day %d: pass anchors, or a quality" % (who, int(day)))
    return a


def lag_rule_evaluate(model, queries, quality=None, mine=None, k=1, agg="noisy_or", sp_index=None, spt_index=None, batch_size=256,
                      lag_edges=DEFAULT_LAG_EDGES, anchors=None, **kw):
    """extrapolation.T_RED_GNN.rule_evaluate (see there)."""
    from .evaluation import KINDS
    from .extrapolation import KnownObjects, _Batch, check_queries
    from .utils import cal_ranks_csr
    who = "rule_evaluate"
    _check_agg(agg, who)
    if (quality is None) == (mine is None):
        raise ValueError("%s: give exactly one of quality (a LagRuleQuality) and mine (queries to mine the rules from)" % who)
    _check_count(k, who, "k", engine.PATHS_MAX_K)
    q = check_queries(model, queries, batch_size, who)
    for name, index in (("sp_index", sp_index), ("spt_index", spt_index)):
        if index is not None and not isinstance(index, KnownObjects):
            raise ValueError("%s: %s must be a KnownObjects index (extrapolation.known_objects_index)" % (who, name))
    if quality is None:
        table = model.rules_all(check_queries(model, mine, 1, who + " (mine)"), k, lag_edges=lag_edges)
        if anchors is None:
            anchors = anchors_before(model.default_anchors(), (q[:, 3] // model.time_granularity).min(), who)
        quality = model.rule_quality(table, anchors)
    _lag_quality(model, quality, who)
    device = model.linear_classifier.weight.device
    to = lambda a: torch.as_tensor(a).to(device)
    ranks, covered = {sfx: [] for sfx in KINDS.values()}, 0
    for lo in range(0, len(q), int(batch_size)):
        b = q[lo:lo + int(batch_size)]
        rs = lag_rule_scores(model, quality, _Batch(b[:, 0], b[:, 1], b[:, 3]), who=who, **kw)
        score = rs.score(agg).contiguous()
        tails = to(b[:, 2].astype(np.int32))
        ans_ptr = torch.arange(len(b) + 1, dtype=torch.int32, device=device)
        for sfx, index in (("", None), ("_fil_t", spt_index), ("_fil", sp_index)):
            keys_of = b[:, 0] if index is None else index.query_keys(b[:, 0], b[:, 1], b[:, 3])
            filt_ptr, filt_idx = temporal_filter_lists(keys_of, b[:, 2], index)
            ranks[sfx].append(cal_ranks_csr(score, ans_ptr, tails, to(filt_ptr), to(filt_idx)).double())
        covered += int((rs.fired.gather(1, tails.long()[:, None]) > 0).sum())
    return _rule_metrics(ranks, covered, len(q))


def _table(key, support, fixed, n_rel):
    """RuleTable of rows key int64 [P, 1 + L] = (head, body) with their counts and fixed-point sums, equal keys merged."""
    if key.shape[0] == 0:
        z = torch.zeros(0, dtype=torch.int64, device=key.device)
        return RuleTable(z, key[:, 1:], z, z.clone(), n_rel)
    uniq, inv = torch.unique(key, dim=0, sorted=True, return_inverse=True)
    zero = torch.zeros(uniq.shape[0], dtype=torch.int64, device=key.device)
    return RuleTable(uniq[:, 0].contiguous(), uniq[:, 1:].contiguous(), zero.index_add(0, inv, support), zero.index_add(0, inv, fixed),
                     n_rel)


def _path_query_rels(who, paths, q_rel, n_rel, n_ids, n_ids_text):
    """(q int64 [B] on the paths' device, n_rel as int): one query relation in 0..n_ids-1 per row of a PathSet, or ValueError."""
    B = paths.edge.shape[0]
    q = torch.as_tensor(_ids(q_rel, "q_rel")).to(paths.edge.device)
    if q.numel() != B:
        raise ValueError("%s: %d query relations for %d rows" % (who, q.numel(), B))
    if int(n_rel) < 1 or (B > 0 and (int(q.min()) < 0 or int(q.max()) >= n_ids)):
        raise ValueError("%s: query relation id out of range (%s=%d)" % (who, n_ids_text, n_ids))
    return q, int(n_rel)


def _path_rules(paths, q, steps):
    """(key int64 [P, 1 + W], support, fixed int64 [P]) of the P present paths of a PathSet: row b's paths have the key (q[b],
    steps[b, j]), ``steps`` int64 [B, k, W]; every path counts once, with its product rounded once, in float64, to
    floor(p * 2^32 + 0.5) units of 2^-32."""
    B, k = paths.edge.shape[:2]
    have = torch.arange(k, device=q.device)[None, :] < paths.count.long()[:, None]          # [B, k]
    key = torch.cat([q[:, None, None].expand(B, k, 1), steps], -1)[have]
    fixed = torch.floor(paths.product[have] * 2.0 ** FRACTION_BITS + 0.5).long()
    return key, torch.ones_like(fixed), fixed


def _step_keys(rel, step):
    """int64 [B, k, 2L]: (r_1, s_1, .., r_L, s_L) of every path, from its relations and second ids [B, k, L] each."""
    return torch.stack([rel, step], 3).reshape(*rel.shape[:2], 2 * rel.shape[2])


def rules_from_paths(paths, q_rel, n_rel):
    """The RuleTable of a PathSet: every present path of row b counts once for the rule (q_rel[b], its relation sequence), with its
    product rounded once, in float64, to floor(p * 2^32 + 0.5) units of 2^-32.  ``q_rel``: one query relation per row."""
    q, n_rel = _path_query_rels("rules_from_paths", paths, q_rel, n_rel, 2 * int(n_rel) + 1, "2*n_rel+1")
    return _table(*_path_rules(paths, q, paths.rels()), n_rel)


def temporal_rules_from_paths(paths, q_rel, n_rel):
    """The TemporalRuleTable of a PathSet of a temporal r-digraph: every present path of row b counts once for the rule (q_rel[b],
    its steps' (relation, direction)), the directions read from paths.digraph.direction() and an identity step (relation ``n_rel``)
    written as direction 3; products rounded as rules_from_paths rounds them.  ``q_rel``: one query relation per row."""
    q, n_rel = _path_query_rels("temporal_rules_from_paths", paths, q_rel, n_rel, int(n_rel) + 1, "n_rel+1")
    rel = paths.rels()
    d = paths._gather(paths.digraph.direction().long(), -1)
    d = torch.where(rel == n_rel, torch.full_like(d, DIRECTION_ANY), d)
    return TemporalRuleTable._merged(*_path_rules(paths, q, _step_keys(rel, d)), n_rel)


def lag_rules_from_paths(paths, q_rel, n_rel, lag_edges):
    """The LagRuleTable of a PathSet of an extrapolation r-digraph: every present path of row b counts once for the rule (q_rel[b],
    its steps' (relation, lag bin)), the lags read from paths.digraph.lag() and binned as profile.lag_bins bins them, an identity step
    (relation ``n_rel``, the model's n_rel_true) written as ANY; products rounded as rules_from_paths rounds them.  ``q_rel``: one
    query relation per row."""
    edges = check_lag_edges(lag_edges)
    q, n_rel = _path_query_rels("lag_rules_from_paths", paths, q_rel, n_rel, int(n_rel) + 1, "n_rel+1")
    rel = paths.rels()
    lag = paths._gather(paths.digraph.lag().long(), 0)
    b = torch.bucketize(lag, torch.tensor(edges, dtype=torch.int64, device=q.device), right=True)      # profile.lag_bins: side="right"
    b = torch.where(rel == n_rel, torch.full_like(b, len(edges) + 1), b)
    return LagRuleTable._merged(*_path_rules(paths, q, _step_keys(rel, b)), edges, n_rel)


def rules(model, subs, rels, objs=None, k=1, mode="test", min_alpha=0.0):
    """RED_GNN_trans.rules (see there)."""
    rd = model.explain(subs, rels, objs, mode=mode, min_alpha=min_alpha)
    return rules_from_paths(rd.top_paths(k), rels, model.n_rel)


def split_rows(loader, data="test", max_queries=None):
    """(subs, rels, objs int64 arrays, mode): one row per (h, r, answer) of the first ``max_queries`` queries of the valid or test
    split, the answers of a query in ascending order."""
    if data not in ("valid", "test"):
        raise ValueError("rules: data must be 'valid' or 'test' (got %r)" % (data,))
    query, answer = (loader.valid_q, loader.valid_a) if data == "valid" else (loader.test_q, loader.test_a)
    n = len(query) if max_queries is None else min(len(query), int(max_queries))
    if n <= 0:
        raise ValueError("rules: no queries in the %s split (n=%d)" % (data, n))
    rows = [(int(query[i][0]), int(query[i][1]), int(o)) for i in range(n) for o in sorted(int(x) for x in answer[i])]
    if not rows:
        raise ValueError("rules: the first %d queries of the %s split have no answers" % (n, data))
    rows = np.array(rows, dtype=np.int64)
    mode = loader.eval_mode(data) if hasattr(loader, "eval_mode") else data
    return rows[:, 0], rows[:, 1], rows[:, 2], mode


def split_rules(model, loader, data="test", k=1, batch=50, max_queries=None):
    """BaseModel.rules: the rule tables of the split's rows (split_rows), walked in batches of ``batch`` rows and added."""
    subs, rels, objs, mode = split_rows(loader, data, max_queries)
    if batch <= 0:
        raise ValueError("rules: batch must be positive (got %d)" % batch)
    table = None
    for lo in range(0, len(subs), batch):
        part = model.rules(subs[lo:lo + batch], rels[lo:lo + batch], objs[lo:lo + batch], k=k, mode=mode)
        table = part if table is None else table + part
    return table


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
    return RDigraph(edges=edges, alpha=alpha, offsets=offsets, reached=reached, score=score, n_hops=L,
                    q_sub=torch.as_tensor(subs_h, dtype=torch.int64).to(device), q_rel=q_rel.clone(), n_rel=int(model.n_rel))


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
                    q_time=q_time.clone(), q_sub=torch.as_tensor(heads_h, dtype=torch.int64).to(device), q_rel=kept[0]["q_rel"].clone(),
                    n_rel=int(model.n_rel), n_time=int(model.n_time))


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
                    q_time=q_time.clone(), data_row=data_row, q_sub=torch.as_tensor(src, dtype=torch.int64).to(device),
                    q_rel=kept[0]["q_rel"].clone(), n_rel=int(model.n_rel_true))


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


# ---- explanation fidelity: answers re-scored on an edited r-digraph ----------------------------------------------------------------
@dataclass
class Rescore:
    """An answer re-scored on its r-digraph with some edges taken away (RDigraph.rescore).  Tensors on the digraph's device.

    score    float32 [B]  the model's score of o on the kept digraph, exactly 0 where o is not reached
    reached  bool [B]     o still has a length-L walk from s through kept edges
    live     bool [E]     the edge is kept AND its head is visited at hop - 1 (a forward sweep from s); only live edges carry messages
    alpha    float32 [E]  the attention recomputed on the edited digraph, 0 for dead edges
    """
    score: torch.Tensor
    reached: torch.Tensor
    live: torch.Tensor
    alpha: torch.Tensor


@dataclass
class Fidelity:
    """How much of an answer's score its best paths carry (model.fidelity).  Tensors on the device.

    score            float32 [B]     the model's score of o (RDigraph.score)
    without          float32 [B, k]  ... with the facts of the row's best j paths deleted, j = 1..k (both directions, every hop)
    only             float32 [B, k]  ... with only the facts of the best j paths, and every self-loop, kept
    reached_without  bool [B, k]     o is still reached after the deletion
    reached_only     bool [B, k]     o is reached through the kept facts
    count            int32 [B]       paths found for the row (<= k); for j past it a row repeats its value at j = count
    paths            PathSet         the paths, with the digraph they index
    """
    score: torch.Tensor
    without: torch.Tensor
    only: torch.Tensor
    reached_without: torch.Tensor
    reached_only: torch.Tensor
    count: torch.Tensor
    paths: PathSet

    def necessity(self):
        """float32 [B, k]: score - without, what the answer loses when the best j paths' facts go (comprehensiveness)."""
        return self.score[:, None] - self.without

    def sufficiency_gap(self):
        """float32 [B, k]: score - only, what the best j paths' facts alone fail to reproduce (0: they are sufficient)."""
        return self.score[:, None] - self.only

    def format(self):
        """One line per row: the score, then per j the score without and with only the best j paths (``x``: o no longer reached)."""
        sc, wo, on = self.score.cpu().tolist(), self.without.cpu().tolist(), self.only.cpu().tolist()
        rw, ro, cnt = self.reached_without.cpu().tolist(), self.reached_only.cpu().tolist(), self.count.cpu().tolist()
        cell = lambda v, ok: "%.4f" % v if ok else "x"
        return ["row %d: score %.4f paths %d  without %s  only %s" % (b, sc[b], cnt[b], " ".join(cell(v, ok) for v, ok in zip(wo[b], rw[b])),
                                                                      " ".join(cell(v, ok) for v, ok in zip(on[b], ro[b])))
                for b in range(len(sc))]


def _has_times(rd):
    """The digraph carries a temporal field: it is not a static one, whatever else it is."""
    return rd.time is not None or rd.q_time is not None or rd.data_row is not None


def _check_static_digraph(rd, who):
    """The host checks of a static r-digraph's tensors (ValueError naming the argument); returns (E, B)."""
    if _has_times(rd):
        raise ValueError("%s: a temporal r-digraph (time is set) is out of scope here; static and inductive models only" % who)
    return _check_digraph_tensors(rd, who)


_X_FIELDS = ("data_row", "time", "q_time", "q_sub", "q_rel", "n_rel")


def _is_extrapolation(rd):
    """The digraph has data rows and no time ids: the extrapolation form (extrapolation.T_RED_GNN.explain)."""
    return rd.data_row is not None and rd.n_time is None


def _check_temporal_fields(rd, who):
    """A temporal r-digraph is a temporal interpolation one, as temporal.T_RED_GNN.explain returns it - every field rescore and
    fact_mask read is set and there are no data rows - or an extrapolation one, as extrapolation.T_RED_GNN.explain returns it: data
    rows, the fields of _X_FIELDS and no n_time (ValueError naming what is missing); both data_row and n_time is a mix of the two.
    No tensor is read."""
    if rd.data_row is not None and rd.n_time is not None:
        raise ValueError("%s: a temporal r-digraph with data_row set is an extrapolation digraph, which is out of scope; temporal "
                         "interpolation (temporal.T_RED_GNN.explain) only" % who)
    if rd.data_row is not None:
        missing = [name for name in _X_FIELDS if getattr(rd, name) is None]
        if missing:
            raise ValueError("%s: an extrapolation r-digraph needs data_row, time, q_time, q_sub, q_rel and n_rel, as "
                             "extrapolation.T_RED_GNN.explain sets them (missing: %s)" % (who, ", ".join(missing)))
        return
    missing =[name for name in ("time", "q_time", "q_sub", "q_rel", "n_rel", "n_time") if getattr(rd, name) is None]
    if missing:
        raise ValueError("%s: a temporal r-digraph needs time, q_time, q_sub, q_rel, n_rel and n_time, as temporal.T_RED_GNN.explain "
                         "sets them (missing: %s)" % (who, ", ".join(missing)))


def _check_temporal_digraph(rd, who):
    """The host checks of a temporal interpolation r-digraph: its fields (_check_temporal_fields), then the tensors (ValueError
    naming the argument); returns (E, B)."""
    _check_temporal_fields(rd, who)
    E, B = _check_digraph_tensors(rd, who)
    if isinstance(rd.n_time, (bool, np.bool_)) or not isinstance(rd.n_time, (int, np.integer)) or rd.n_time < 1:
        raise ValueError("%s: n_time must be a positive integer (got %r)" % (who, rd.n_time))
    t, q = rd.time, rd.q_time
    if not torch.is_tensor(t) or t.dtype != torch.int32 or t.shape != (E,):
        raise ValueError("%s: time must be int32 [%d], one per edge" % (who, E))
    if not torch.is_tensor(q) or q.dtype != torch.int32 or q.shape != (B,):
        raise ValueError("%s: q_time must be int32 [%d], one per row" % (who, B))
    for name, x in (("time", t), ("q_time", q)):
        if x.numel() and (int(x.min()) < 0 or int(x.max()) >= rd.n_time):
            raise ValueError("%s: %s holds a time id outside 0..%d" % (who, name, rd.n_time - 1))
    return E, B


def _check_extrapolation_digraph(rd, who):
    """The host checks of an extrapolation r-digraph: its fields (ValueError naming extrapolation.T_RED_GNN.explain where it is not
    one), then the tensors' types and shapes; returns (E, B).  Only q_time, one entry per row, is read."""
    if not _is_extrapolation(rd):
        raise ValueError("%s: not an extrapolation r-digraph (data_row set and n_time None, as extrapolation.T_RED_GNN.explain returns it)"
                         % who)
    _check_temporal_fields(rd, who)
    E, B = _check_digraph_tensors(rd, who)
    for name, n, what in (("time", E, "edge"), ("data_row", E, "edge"), ("q_time", B, "row")):
        t = getattr(rd, name)
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.shape != (n,):
            raise ValueError("%s: %s must be int32 [%d], one per %s" % (who, name, n, what))
    if B and int(rd.q_time.min()) < 0:
        raise ValueError("%s: q_time holds a negative day" % who)
    return E, B


def _check_digraph_tensors(rd, who):
    """edges, alpha, offsets, n_hops and n_rel of any r-digraph; returns (E, B)."""
    if isinstance(rd.n_hops, (bool, np.bool_)) or not isinstance(rd.n_hops, (int, np.integer)) or not 1 <= rd.n_hops <= 32:
        raise ValueError("%s: n_hops must be an integer in 1..32 (got %r)" % (who, rd.n_hops))
    e, a, o = rd.edges, rd.alpha, rd.offsets
    if not all(torch.is_tensor(t) for t in (e, a, o)):
        raise ValueError("%s: edges, alpha and offsets must be tensors" % who)
    if e.dtype != torch.int32 or e.dim() != 2 or e.shape[1] != 5:
        raise ValueError("%s: edges must be int32 [E, 5] (got %s %s)" % (who, e.dtype, tuple(e.shape)))
    if a.dtype != torch.float32 or a.shape != (e.shape[0],):
        raise ValueError("%s: alpha must be float32 [%d] (got %s %s)" % (who, e.shape[0], a.dtype, tuple(a.shape)))
    if o.dtype != torch.int64 or o.dim() != 1 or o.numel() < 1:
        raise ValueError("%s: offsets must be int64 [B + 1] (got %s %s)" % (who, o.dtype, tuple(o.shape)))
    off = o.detach().cpu().numpy()
    if off[0] != 0 or off[-1] != e.shape[0] or (np.diff(off) < 0).any():
        raise ValueError("%s: offsets must start at 0, never decrease and end at the number of edges (%d)" % (who, e.shape[0]))
    if isinstance(rd.n_rel, (bool, np.bool_)) or not isinstance(rd.n_rel, (int, np.integer)) or rd.n_rel < 1:
        raise ValueError("%s: n_rel must be a positive integer (got %r); model.explain sets it" % (who, rd.n_rel))
    return e.shape[0], o.numel() - 1


def fact_mask(rd, facts, rows=None, inverse_offset=None):
    """RDigraph.fact_mask (see there)."""
    who = "fact_mask"
    timed, xtr = _has_times(rd), _is_extrapolation(rd)
    E, B = (_check_extrapolation_digraph if xtr else _check_temporal_digraph)(rd, who) if timed else _check_static_digraph(rd, who)
    dev = rd.edges.device
    f = (facts.detach() if torch.is_tensor(facts) else torch.as_tensor(np.asarray(facts))).to(dev)
    n_rel = int(rd.n_rel)
    if timed:
        if f.is_floating_point() or f.dtype == torch.bool or f.dim() != 2 or f.shape[1] != 4:
            raise ValueError("%s: on a temporal r-digraph facts must be integers [F, 4] = (h, r, t, %s) (got %s %s)"
                             % (who, "day" if xtr else "time id", f.dtype, tuple(f.shape)))
        f = f.long()
        if f.shape[0] and (int(f.min()) < 0 or int(f[:, 1].max()) > n_rel):
            raise ValueError("%s: facts hold a negative id%s or a relation above n_rel = %d" % (who, " or day" if xtr else "", n_rel))
        if not xtr and f.shape[0] and int(f[:, 3].max()) >= rd.n_time:
            raise ValueError("%s: facts hold a time id outside 0..%d" % (who, rd.n_time - 1))
        m = inverse_offset
        if m is not None and (isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 1 or 2 * m > n_rel):
            raise ValueError("%s: inverse_offset must be an integer m with 1 <= m and 2 m <= n_rel = %d, relation r's inverse being r + m "
                             "below m and r - m from there on (got %r)" % (who, n_rel, m))
    else:
        if inverse_offset is not None:
            raise ValueError("%s: inverse_offset is for temporal r-digraphs; a static one knows its inverses (r + n_rel)" % who)
        if f.is_floating_point() or f.dtype == torch.bool or f.dim() != 2 or f.shape[1] != 3:
            raise ValueError("%s: facts must be integers [F, 3] = (h, r, t) (got %s %s)" % (who, f.dtype, tuple(f.shape)))
        f = f.long()
        if f.shape[0] and (int(f.min()) < 0 or int(f[:, 1].max()) > 2 * n_rel):
            raise ValueError("%s: facts hold a negative id or a relation above 2*n_rel = %d" % (who, 2 * n_rel))
    r_of = None
    if rows is not None:
        r_of = (rows.detach() if torch.is_tensor(rows) else torch.as_tensor(np.asarray(rows))).to(dev)
        if r_of.is_floating_point() or r_of.dtype == torch.bool or r_of.shape != (f.shape[0],):
            raise ValueError("%s: rows must be integers [%d], one per fact (got %s %s)" % (who, f.shape[0], r_of.dtype, tuple(r_of.shape)))
        r_of = r_of.long()
        if r_of.numel() and (int(r_of.min()) < 0 or int(r_of.max()) >= B):
            raise ValueError("%s: rows out of range (the digraph has %d rows)" % (who, B))
    mask = torch.zeros(E, dtype=torch.bool, device=dev)
    if timed:
        fact = f[:, 1] != n_rel                           # the identity is no fact
        f = f[fact]
        if E == 0 or f.shape[0] == 0:
            return mask
        e = rd.edges.long()
        n_key = int(max(e[:, 2].max(), e[:, 4].max(), f[:, 0].max(), f[:, 2].max())) + 1
        # (an extrapolation digraph has days, not time ids: the key takes the largest one at hand)
        n_r, n_t = n_rel + 1, int(max(rd.time.max(), f[:, 3].max())) + 1 if xtr else int(rd.n_time)
        key = lambda row, h, r, t, tm: (((row * n_key + h) * n_r + r) * n_key + t) * n_t + tm
        f_row = torch.zeros_like(f[:, 0]) if r_of is None else r_of[fact]
        e_row = torch.zeros_like(e[:, 0]) if r_of is None else e[:, 0]
        want = key(f_row, f[:, 0], f[:, 1], f[:, 2], f[:, 3])
        if inverse_offset is not None:
            m = int(inverse_offset)
            want = torch.cat([want, key(f_row, f[:, 2], torch.where(f[:, 1] < m, f[:, 1] + m, f[:, 1] - m), f[:, 0], f[:, 3])])
        hit = torch.isin(key(e_row, e[:, 2], e[:, 3], e[:, 4], rd.time.long()), want) & (e[:, 3] != n_rel)
        return hit & (rd.data_row.to(dev) >= 0) if xtr else hit       # a self-loop has no data row and is never a fact
    fact = f[:, 1] != 2 * n_rel                           # the identity is no fact
    f = f[fact]
    if E == 0 or f.shape[0] == 0:
        return mask
    e = rd.edges.long()
    n_key = int(max(e[:, 2].max(), e[:, 4].max(), f[:, 0].max(), f[:, 2].max())) + 1
    n_r = 2 * n_rel + 1
    key = lambda row, h, r, t: ((row * n_key + h) * n_r + r) * n_key + t
    inv = torch.where(f[:, 1] < n_rel, f[:, 1] + n_rel, f[:, 1] - n_rel)
    f_row = torch.zeros_like(f[:, 0]) if r_of is None else r_of[fact]
    e_row = torch.zeros_like(e[:, 0]) if r_of is None else e[:, 0]
    want = torch.cat([key(f_row, f[:, 0], f[:, 1], f[:, 2]), key(f_row, f[:, 2], inv, f[:, 0])])
    return torch.isin(key(e_row, e[:, 2], e[:, 3], e[:, 4]), want) & (e[:, 3] != 2 * n_rel)


def data_row_mask(rd, data_rows, rows=None):
    """RDigraph.data_row_mask (see there)."""
    who = "data_row_mask"
    E, B = _check_extrapolation_digraph(rd, who)
    dev = rd.edges.device
    f = (data_rows.detach() if torch.is_tensor(data_rows) else torch.as_tensor(np.asarray(data_rows))).to(dev)
    if f.is_floating_point() or f.dtype == torch.bool or f.dim() != 1:
        raise ValueError("%s: data_rows must be integers [F] (got %s %s)" % (who, f.dtype, tuple(f.shape)))
    f = f.long()
    if f.numel() and int(f.min()) < 0:
        raise ValueError("%s: data_rows hold a negative row (a self-loop has no data row)" % who)
    row_of = rd.data_row.to(dev).long()
    if rows is None:
        return torch.isin(row_of, f) & (row_of >= 0)
    r_of = (rows.detach() if torch.is_tensor(rows) else torch.as_tensor(np.asarray(rows))).to(dev)
    if r_of.is_floating_point() or r_of.dtype == torch.bool or r_of.shape != (f.shape[0],):
        raise ValueError("%s: rows must be integers [%d], one per data row (got %s %s)" % (who, f.shape[0], r_of.dtype, tuple(r_of.shape)))
    r_of = r_of.long()
    if r_of.numel() and (int(r_of.min()) < 0 or int(r_of.max()) >= B):
        raise ValueError("%s: rows out of range (the digraph has %d rows)" % (who, B))
    n_key = int(max(row_of.max() if E else 0, f.max() if f.numel() else 0)) + 1
    return torch.isin(rd.edges[:, 0].long() * n_key + row_of, r_of * n_key + f) & (row_of >= 0)


def _sorted_find(keys, want):
    """(position int64, found bool) of every ``want`` in the sorted, duplicate-free ``keys``."""
    if keys.numel() == 0:
        return torch.zeros_like(want), torch.zeros_like(want, dtype=torch.bool)
    pos = torch.searchsorted(keys, want).clamp_(max=keys.numel() - 1)
    return pos, keys[pos] == want


def _hop_index(who, l, L, at, row, head, tail, keys_prev, n_ent, live):
    """The index arrays of hop l of a rescore from its kept edges ``at`` (indices into the digraph's edges, in order): the forward
    sweep against the previous hop's sorted node keys (``live`` is marked), then the hop's node list - the sorted unique (row, tail) -
    and its CSR.  Returns None where no edge is live, else (at, src, keys, dst_ptr, row_of, prev_idx, had): the live edges, their
    head's position in ``keys_prev``, the node keys row * n_ent + tail, the CSR of the edges by node (int32), the nodes' rows, and
    each node's position in ``keys_prev`` (int32, -1 where ``had`` is False)."""
    src, ok = _sorted_find(keys_prev, row[at] * n_ent + head[at])
    at, src = at[ok], src[ok]                                         # the forward sweep: the head is visited one hop down
    if at.numel() == 0:
        return None                                                   # nothing is reached from here on: every score stays 0
    live[at] = True
    tk = row[at] * n_ent + tail[at]
    if bool((tk[1:] < tk[:-1]).any()):
        raise ValueError("%s: edges must be ordered by (row, hop, tail), as model.explain returns them" % who)
    keys, counts = torch.unique_consecutive(tk, return_counts=True)   # the hop's node list: sorted unique (row, tail)
    dst_ptr = torch.zeros(keys.numel() + 1, dtype=torch.int32, device=tk.device)
    dst_ptr[1:] = torch.cumsum(counts, 0)
    row_of = keys // n_ent
    if l == L and bool((row_of[1:] == row_of[:-1]).any()):
        raise ValueError("%s: the hop-%d edges of a row must share their tail, the row's answer" % (who, L))
    prev_idx, had = _sorted_find(keys_prev, keys)
    prev_idx = torch.where(had, prev_idx, torch.full_like(prev_idx, -1)).to(torch.int32).contiguous()
    return at, src, keys, dst_ptr, row_of, prev_idx, had


def _check_keep(who, keep, E, device):
    if keep is not None:
        keep = keep if torch.is_tensor(keep) else torch.as_tensor(np.asarray(keep)).to(device)      # (an array goes along)
        if keep.dtype not in (torch.bool, torch.uint8) or keep.shape != (E,):
            raise ValueError("%s: keep must be bool or uint8 [%d], one per edge (got %s %s)" % (who, E, keep.dtype, tuple(keep.shape)))
    return keep


def rescore_temporal(rd, model, keep=None, mode="test", who="rescore", tape=None):
    """RDigraph.rescore of a temporal interpolation digraph (see there): T_RED_GNN._run's layer over the kept edges, hop by hop.
    ``tape``: a list that receives, per hop walked, what the hop's adjoint needs (RDigraph.saliency): the hop, its index arrays, the
    directed tables the kernel read and the sums it formed."""
    from .temporal import T_RED_GNN, eval_semantics
    if not isinstance(model, T_RED_GNN):
        raise ValueError("%s: a temporal r-digraph (time, q_time or data_row is set) is re-scored by the temporal.T_RED_GNN that "
                         "explained it (got %s)" % (who, type(model).__name__))
    E, B = _check_temporal_digraph(rd, who)
    if mode != "test":
        raise ValueError("%s: a temporal r-digraph is explained on the full graph; mode must be 'test' (got %r)" % (who, mode))
    for name in ("q_sub", "q_rel"):
        t = getattr(rd, name)
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.shape != (B,):
            raise ValueError("%s: %s must be int64 [%d], the rows' queries (model.explain sets it)" % (who, name, B))
    L = int(rd.n_hops)
    if model.n_layer != L or model.n_rel != rd.n_rel or model.n_time != rd.n_time:
        raise ValueError("%s: the temporal digraph has n_hops=%d, n_rel=%d, n_time=%d, the model n_layer=%d, n_rel=%d, n_time=%d"
                         % (who, L, rd.n_rel, rd.n_time, model.n_layer, model.n_rel, model.n_time))
    keep = _check_keep(who, keep, E, rd.edges.device)
    dev = rd.edges.device
    tensors = [rd.edges, rd.alpha, rd.offsets, rd.q_sub, rd.q_rel, rd.time, rd.q_time] + ([keep] if keep is not None else [])
    if not all(t.is_cuda for t in tensors) or any(t.device != dev for t in tensors):
        raise ValueError("%s: the layers run in HIP and need the digraph (and keep) on one device (got CPU tensors or mixed devices)" % who)
    n_ent, n_rel = model.n_ent, int(rd.n_rel)
    e = rd.edges.long()
    row, hop, head, rel, tail = e.unbind(1)
    if B and (int(rd.q_sub.min()) < 0 or int(rd.q_sub.max()) >= n_ent or int(rd.q_rel.min()) < 0 or int(rd.q_rel.max()) > n_rel):
        raise ValueError("%s: q_sub / q_rel out of range (n_ent=%d, n_rel+1=%d)" % (who, n_ent, n_rel + 1))
    if E:
        lo, hi = e.min(0).values.tolist(), e.max(0).values.tolist()
        if lo[0] < 0 or hi[0] >= B or lo[1] < 1 or hi[1] > L or min(lo[2], lo[4]) < 0 or max(hi[2], hi[4]) >= n_ent or lo[3] < 0 \
                or hi[3] > n_rel:
            raise ValueError("%s: edges hold a row, hop, entity or relation out of range (B=%d, L=%d, n_ent=%d, n_rel+1=%d)"
                             % (who, B, L, n_ent, n_rel + 1))
    d, a = model.hidden_dim, model.attn_dim
    ld, ap = max(16, _pad4(d)), pad_attn(a)
    i32 = lambda t: t.to(torch.int32).contiguous()
    padc = lambda t: F.pad(t, (0, ld - d)) if ld != d else t
    pad_rows = lambda w: F.pad(w, (0, 0, 0, ap - a)) if ap != a else w
    live = torch.zeros(E, dtype=torch.bool, device=dev)
    alpha = torch.zeros(E, dtype=torch.float32, device=dev)
    score = torch.zeros(B, dtype=torch.float32, device=dev)
    reached = torch.zeros(B, dtype=torch.bool, device=dev)
    kept = torch.ones(E, dtype=torch.bool, device=dev) if keep is None else keep.bool()
    with torch.no_grad(), eval_semantics(model):
        from .models import tall_linear
        # the tables of T_RED_GNN._run, formed the same way
        w_dir = torch.cat([model.past_linear.weight, model.now_linear.weight, model.future_linear.weight], 0)     # [3d, d]
        time_dir = padc(F.linear(model.time_embed.weight, w_dir).view(model.n_time, 3, d).transpose(0, 1).reshape(3 * model.n_time, d)).contiguous()
        zero_b = torch.zeros(1, device=dev)                                   # the temporal attention has no bias
        q_time = rd.q_time.contiguous()
        keys_prev = torch.arange(B, device=dev) * n_ent + rd.q_sub            # hop 0: the node (row, s) of every row, sorted
        hidden = torch.zeros((B, d), device=dev)
        for l in range(1, L + 1):
            at = torch.nonzero((hop == l) & kept).reshape(-1)
            index = _hop_index(who, l, L, at, row, head, tail, keys_prev, n_ent, live)
            if index is None:
                break
            at, src, keys, dst_ptr, row_of, _, _ = index
            rela, w1, w2 = model._tables(l - 1)
            n_old = hidden.shape[0]
            a_s = tall_linear(hidden, pad_rows(w1[:, :d])).contiguous()                   # [n_old, ap]
            a_r = F.linear(rela, pad_rows(w1[:, d:2 * d])).contiguous()                  # [n_rel + 1, ap]
            a_q = F.linear(rela[rd.q_rel], pad_rows(w1[:, 2 * d:])).contiguous()         # [B, ap]
            hidden_dir = padc(tall_linear(hidden, w_dir).view(n_old * 3, d)).contiguous()            # row 3 s + dir
            rela_dir = padc(F.linear(rela, w_dir).view(-1, 3, d).transpose(0, 1).reshape(-1, d)).contiguous()   # row dir * (R + 1) + r
            agg, al = engine.digraph_tlayer_fwd(dst_ptr, i32(src), i32(rel[at]), i32(row_of), hidden_dir, rela_dir, time_dir, d, a_s, a_r,
                                                a_q, w2.reshape(-1).contiguous(), zero_b, a, edge_time=rd.time[at].contiguous(),
                                                q_time=q_time, n_dir=3)
            alpha[at] = al
            if tape is not None:
                tape.append(dict(l=l, at=at, dst_ptr=dst_ptr, src=i32(src), rel=i32(rel[at]), row_of=i32(row_of), hidden=hidden_dir,
                                 rela=rela_dir, time_tab=time_dir, a_s=a_s, a_r=a_r, a_q=a_q, w_alpha=w2.reshape(-1).contiguous(),
                                 b_alpha=zero_b, edge_time=rd.time[at].contiguous(), q_time=q_time, agg=agg, w_dir=w_dir,
                                 w_s=w1[:, :d]))
            hidden = model.act(agg[:, :d])                                    # no GRU, and eval semantics: no dropout
            keys_prev = keys
            if l == L:
                score[row_of] = tall_linear(hidden, model.linear_classifier.weight, model.linear_classifier.bias).reshape(-1)
                reached[row_of] = True
    return Rescore(score=score, reached=reached, live=live, alpha=alpha)


def rescore_extrapolation(rd, model, keep=None, mode="test", who="rescore", tape=None):
    """RDigraph.rescore of an extrapolation digraph (see there): the inference branch of extrapolation.T_RED_GNN._run over the kept
    edges, hop by hop, the per-hop index built in HIP (engine.digraph_hop_index).  ``tape``: as rescore_temporal's."""
    import math
    from .extrapolation import T_RED_GNN as XModel
    from .temporal import eval_semantics
    _check_temporal_fields(rd, who)
    if not isinstance(model, XModel):
        raise ValueError("%s: an extrapolation r-digraph (data_row is set, n_time is not) is re-scored by the extrapolation.T_RED_GNN "
                         "that explained it (got %s)" % (who, type(model).__name__))
    if mode != "test":
        raise ValueError("%s: an extrapolation r-digraph is explained by extrapolation.T_RED_GNN on its own data; mode must be 'test' "
                         "(got %r)" % (who, mode))
    E, B = _check_extrapolation_digraph(rd, who)
    for name in ("q_sub", "q_rel"):
        t = getattr(rd, name)
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.shape != (B,):
            raise ValueError("%s: %s must be int64 [%d], the rows' queries (model.explain sets it)" % (who, name, B))
    L = int(rd.n_hops)
    if model.n_layer != L or model.n_rel_true != rd.n_rel:
        raise ValueError("%s: the extrapolation digraph has n_hops=%d, n_rel=%d, the model n_layer=%d, n_rel=%d"
                         % (who, L, rd.n_rel, model.n_layer, model.n_rel_true))
    keep = _check_keep(who, keep, E, rd.edges.device)
    dev = rd.edges.device
    tensors = [rd.edges, rd.alpha, rd.offsets, rd.q_sub, rd.q_rel, rd.time, rd.q_time, rd.data_row] + ([keep] if keep is not None else [])
    if not all(t.is_cuda for t in tensors) or any(t.device != dev for t in tensors):
        raise ValueError("%s: the layers run in HIP and need the digraph (and keep) on one device (got CPU tensors or mixed devices)" % who)
    n_ent, n_rows = model.n_ent, model.n_rel + 1                             # rows of the relation tables: n_rel_true + 2
    if B and (int(rd.q_sub.min()) < 0 or int(rd.q_sub.max()) >= n_ent or int(rd.q_rel.min()) < 0 or int(rd.q_rel.max()) >= rd.n_rel):
        raise ValueError("%s: q_sub / q_rel out of range (n_ent=%d, n_rel=%d)" % (who, n_ent, rd.n_rel))
    d, a = model.hidden_dim, model.attn_dim
    ld, ap = max(16, _pad4(d)), pad_attn(a)
    padc = lambda t: F.pad(t, (0, ld - d)) if ld != d else t
    pad_rows = lambda w: F.pad(w, (0, 0, 0, ap - a)) if ap != a else w
    live = torch.zeros(E, dtype=torch.uint8, device=dev)
    alpha = torch.zeros(E, dtype=torch.float32, device=dev)
    score = torch.zeros(B, dtype=torch.float32, device=dev)
    reached = torch.zeros(B, dtype=torch.bool, device=dev)
    keep8 = None if keep is None else keep.to(torch.uint8).contiguous()
    edges, edge_time, q_time = rd.edges.contiguous(), rd.time.contiguous(), rd.q_time.contiguous()
    bad = lambda status: engine.digraph_index_error(status, who, L, n_ent, n_rows)
    with torch.no_grad(), eval_semantics(model):
        lin = engine.rows_linear                                              # the tables of T_RED_GNN._run without gradients
        w_past = model.past_linear.weight
        # a lag is at most the query's day (days are not negative), and rows_linear's rows do not depend on the row count: a table
        # over 0 .. the largest query day holds the forward's rows for every lag of the digraph, without a pass over the edges
        n_tab = int(q_time.max()) + 1 if B else 1
        deltas = torch.arange(n_tab, dtype=torch.float32, device=dev)
        z = 2 * math.pi * model.time_embed.periodic.weight * deltas.view(-1, 1)
        pos = model.time_embed.linear_pos
        t_emb = torch.relu(lin(torch.cat([torch.cos(z), torch.sin(z)], -1), pos.weight[0].t(), pos.bias[0]))
        time_p = padc(lin(t_emb, w_past)).contiguous()
        zero_b = torch.zeros(1, device=dev)                                   # the attention has no bias
        ranges = engine.digraph_hop_ranges(edges, rd.offsets.contiguous(), L)
        if ranges.status:
            raise bad(ranges.status)
        keys_prev = torch.arange(B, device=dev) * n_ent + rd.q_sub            # hop 0: the node (row, s) of every row, sorted
        hidden = torch.zeros((B, d), device=dev)
        for l in range(1, L + 1):
            at, src, rel, tm, keys, dst_ptr, row_of, _, status = engine.digraph_hop_index(edges, ranges, l, keys_prev, n_ent, n_rows, live,
                                                                                         keep8, edge_time)
            if status:
                raise bad(status)
            if at.numel() == 0:
                break                                                         # nothing is reached from here on: every score stays 0
            rela, w1, w2 = model.rela_embed_layer[l - 1].weight, model.attention_1_layer[l - 1].weight, model.attention_2_layer[l - 1].weight
            a_s = lin(hidden, pad_rows(w1[:, :d])).contiguous()
            a_r = F.linear(rela, pad_rows(w1[:, d:2 * d])).contiguous()
            a_q = lin(rela[rd.q_rel], pad_rows(w1[:, 2 * d:])).contiguous()
            hidden_p = padc(lin(hidden, w_past)).contiguous()
            rela_p = padc(F.linear(rela, w_past)).contiguous()
            agg, al = engine.digraph_tlayer_fwd(dst_ptr, src, rel, row_of, hidden_p, rela_p, time_p, d, a_s, a_r, a_q,
                                                w2.reshape(-1).contiguous(), zero_b, a, edge_time=tm, q_time=q_time, n_dir=1,
                                                dst_ptr_host=dst_ptr.cpu().numpy())      # the hop's one copy: the kernel cuts hubs there
            alpha[at.long()] = al
            if tape is not None:
                tape.append(dict(l=l, at=at.long(), dst_ptr=dst_ptr, src=src, rel=rel, row_of=row_of, hidden=hidden_p, rela=rela_p,
                                 time_tab=time_p, a_s=a_s, a_r=a_r, a_q=a_q, w_alpha=w2.reshape(-1).contiguous(), b_alpha=zero_b,
                                 edge_time=tm, q_time=q_time, agg=agg, w_dir=w_past, w_s=w1[:, :d]))
            hidden = model.act(agg[:, :d])
            keys_prev = keys
            if l == L:
                cls = model.linear_classifier
                score[row_of.long()] = lin(hidden, cls.weight, cls.bias).reshape(-1)
                reached[row_of.long()] = True
    return Rescore(score=score, reached=reached, live=live.bool(), alpha=alpha)


def extrapolation_fidelity(model, X, objs=None, k=4, inverse_offset=None):
    """extrapolation.T_RED_GNN.fidelity (see there)."""
    _check_count(k, "fidelity", "k", engine.PATHS_MAX_K)
    rd = model.explain(X, objs)
    return _fidelity_of(rd, model, k, rd.edges[:, 3] == model.n_rel_true, "test", inverse_offset)


def extrapolation_fidelity_all(model, queries, k=4, batch_size=64, inverse_offset=None):
    """extrapolation.T_RED_GNN.fidelity_all (see there)."""
    from .extrapolation import _Batch, check_queries
    _check_count(k, "fidelity_all", "k", engine.PATHS_MAX_K)
    q = check_queries(model, queries, batch_size, "fidelity_all")
    parts = []
    for lo in range(0, len(q), int(batch_size)):
        b = q[lo:lo + int(batch_size)]
        parts.append(model.fidelity(_Batch(b[:, 0], b[:, 1], b[:, 3]), b[:, 2], k=int(k), inverse_offset=inverse_offset))
    return _fidelity_summary(parts, k)


def rescore(rd, model, keep=None, mode="test", gate=None):
    """RDigraph.rescore (see there)."""
    who = "rescore"
    if gate is not None:
        return _gated_call(rd, model, keep, mode, gate, who, False)
    if _is_extrapolation(rd):
        return rescore_extrapolation(rd, model, keep, mode)
    if _has_times(rd):
        return rescore_temporal(rd, model, keep, mode)
    return _rescore_static(rd, model, keep, mode, who)


def _static_setup(rd, model, keep, mode, who):
    """The checks every walk of a static r-digraph starts with (ValueError), and what they establish: a namespace of the sizes, the
    edge columns as int64, the kept edges and the padded widths."""
    E, B = _check_static_digraph(rd, who)
    for name in ("q_sub", "q_rel"):
        t = getattr(rd, name)
        if not torch.is_tensor(t) or t.dtype != torch.int64 or t.shape != (B,):
            raise ValueError("%s: %s must be int64 [%d], the rows' queries (model.explain sets it)" % (who, name, B))
    for name in ("n_layer", "hidden_dim", "attn_dim", "gnn_layers", "W_final", "gate", "loader"):
        if not hasattr(model, name):
            raise ValueError("%s: model must be a RED_GNN_trans or RED_GNN_induc (got %s)" % (who, type(model).__name__))
    L = int(rd.n_hops)
    if model.n_layer != L or model.n_rel != rd.n_rel:
        raise ValueError("%s: the digraph has n_hops=%d, n_rel=%d, the model n_layer=%d, n_rel=%d" % (who, L, rd.n_rel, model.n_layer,
                                                                                                    model.n_rel))
    keep = _check_keep(who, keep, E, rd.edges.device)
    dev = rd.edges.device
    tensors = [rd.edges, rd.alpha, rd.offsets, rd.q_sub, rd.q_rel] + ([keep] if keep is not None else [])
    if not all(t.is_cuda for t in tensors) or any(t.device != dev for t in tensors):
        raise ValueError("%s: the layers run in HIP and need the digraph (and keep) on one device (got CPU tensors or mixed devices)" % who)
    n_ent = model.loader.graph_for(mode).n_ent
    e = rd.edges.long()
    row, hop, head, rel, tail = e.unbind(1)
    if B and (int(rd.q_sub.min()) < 0 or int(rd.q_sub.max()) >= n_ent or int(rd.q_rel.min()) < 0 or int(rd.q_rel.max()) > 2 * rd.n_rel):
        raise ValueError("%s: q_sub / q_rel out of range (n_ent=%d, 2*n_rel+1=%d)" % (who, n_ent, 2 * rd.n_rel + 1))
    if E:
        lo, hi = e.min(0).values.tolist(), e.max(0).values.tolist()
        if lo[0] < 0 or hi[0] >= B or lo[1] < 1 or hi[1] > L or min(lo[2], lo[4]) < 0 or max(hi[2], hi[4]) >= n_ent or lo[3] < 0 \
                or hi[3] > 2 * rd.n_rel:
            raise ValueError("%s: edges hold a row, hop, entity or relation out of range (B=%d, L=%d, n_ent=%d in mode %r, 2*n_rel+1=%d)"
                             % (who, B, L, n_ent, mode, 2 * rd.n_rel + 1))
    d, a = model.hidden_dim, model.attn_dim
    ld, ap = max(16, _pad4(d)), pad_attn(a)
    fused = model.fused_dense and engine.dense_supported(d, a)
    kept = torch.ones(E, dtype=torch.bool, device=dev) if keep is None else keep.bool()
    return types.SimpleNamespace(E=E, B=B, L=L, dev=dev, n_ent=n_ent, row=row, hop=hop, head=head, rel=rel, tail=tail, d=d, a=a, ld=ld,
                                 ap=ap, fused=fused, kept=kept)


def _rescore_static(rd, model, keep, mode, who, tape=None):
    """RDigraph.rescore of a static r-digraph for ``who`` (rescore, saliency).  ``tape``: a list that receives, per hop walked, what the
    hop's adjoint needs (RDigraph.saliency): the hop, its index arrays, the state and projection it read and the sums it formed."""
    S = _static_setup(rd, model, keep, mode, who)
    E, B, L, dev, n_ent, d, a, ld, ap, fused, kept = S.E, S.B, S.L, S.dev, S.n_ent, S.d, S.a, S.ld, S.ap, S.fused, S.kept
    row, hop, head, rel, tail = S.row, S.hop, S.head, S.rel, S.tail
    i32 = lambda t: t.to(torch.int32).contiguous()
    live = torch.zeros(E, dtype=torch.bool, device=dev)
    alpha = torch.zeros(E, dtype=torch.float32, device=dev)
    score = torch.zeros(B, dtype=torch.float32, device=dev)
    reached = torch.zeros(B, dtype=torch.bool, device=dev)
    with torch.no_grad():
        from .models import gru_step, tall_linear
        tables = model.inference_tables(rd.q_rel.contiguous(), ld, ap)
        keys_prev = torch.arange(B, device=dev) * n_ent + rd.q_sub            # hop 0: the node (row, s) of every row, sorted
        hidden = torch.zeros((B, ld), device=dev)
        a_s = torch.zeros((B, ap), device=dev)                                # hidden == 0 at layer 0
        for l in range(1, L + 1):
            layer, last = model.gnn_layers[l - 1], l == L
            at = torch.nonzero((hop == l) & kept).reshape(-1)
            index = _hop_index(who, l, L, at, row, head, tail, keys_prev, n_ent, live)
            if index is None:
                break                                                         # nothing is reached from here on: every score stays 0
            at, src, keys, dst_ptr, row_of, prev_idx, had = index
            a_r, a_q, rela_p = tables[l - 1]
            agg, al = engine.digraph_layer_fwd(dst_ptr, i32(src), i32(rel[at]), i32(row_of), hidden, rela_p.contiguous(), d, a_s,
                                               a_r.contiguous(), a_q.contiguous(), layer.w_alpha.weight.detach().reshape(-1).contiguous(),
                                               layer.w_alpha.bias.detach().contiguous(), a)
            alpha[at] = al
            if tape is not None:
                tape.append(dict(l=l, at=at, dst_ptr=dst_ptr, src=i32(src), rel=i32(rel[at]), row_of=i32(row_of), hidden=hidden, a_s=a_s,
                                 agg=agg, prev_idx=prev_idx, had=had, a_r=a_r.contiguous(), a_q=a_q.contiguous(),
                                 rela=rela_p.contiguous()))
            if fused:                                                         # the dense step of _forward_inference
                node_rows = torch.stack([row_of, torch.zeros_like(row_of)], 1).to(torch.int32).contiguous()
                hidden, a_s = engine.dense_fwd(agg, hidden, prev_idx, d, layer.W_h.weight, model.act_name, model.gate,
                                               Ws_next=None if last else model.gnn_layers[l].Ws_attn.weight, attn_dim=a, ap=ap,
                                               W_final=model.W_final.weight if last else None, nodes=node_rows, n_ent=1,
                                               scores_all=score, precision=model.dense_precision, want_hidden=not last)
            else:                                                             # ... and of _run's ``kept`` branch
                x = layer.act(tall_linear(agg[:, :d], layer.W_h.weight))
                h0 = torch.zeros((keys.numel(), d), device=dev)
                h0[had] = hidden[:, :d][prev_idx[had].long()]
                hid = gru_step(x, h0, model.gate)
                if last:
                    score[row_of] = tall_linear(hid, model.W_final.weight).squeeze(-1)
                else:
                    w_s = model.gnn_layers[l].Ws_attn.weight
                    a_s = tall_linear(hid, F.pad(w_s, (0, 0, 0, ap - a)) if ap != a else w_s).contiguous()
                    hidden = (F.pad(hid, (0, ld - d)) if ld != d else hid).contiguous()
            if last:
                reached[row_of] = True
            keys_prev = keys
    return Rescore(score=score, reached=reached, live=live, alpha=alpha)


def _segment_max(values, group, n_groups):
    """float32 [n_groups]: the largest of ``values`` per ``group`` (int64); 0 for a group without values."""
    out = torch.zeros(n_groups, dtype=torch.float32, device=values.device)
    return out.scatter_reduce(0, group, values, "amax", include_self=False) if values.numel() else out


def _segment_sums(values, group, n_groups):
    """float32 [n_groups]: the sum of ``values`` per ``group`` (int64, never decreasing), each group's values added in a fixed order -
    laid out as one matrix row per group and summed along it, no atomics: the same bits on every run."""
    out = torch.zeros(n_groups, dtype=torch.float32, device=values.device)
    if values.numel() == 0:
        return out
    counts = torch.bincount(group, minlength=n_groups)
    first = torch.cumsum(counts, 0) - counts
    m = torch.zeros((n_groups, int(counts.max())), dtype=torch.float32, device=values.device)
    m[group, torch.arange(group.numel(), device=group.device) - first[group]] = values
    return m.sum(1)


class _FactSums:
    """Per-edge values of an r-digraph summed per fact: the grouping Saliency (``edge_grad``) and Attribution (``edge_attr``) share.  A
    subclass names its per-edge field in ``_VALUES`` and has ``digraph``, ``score`` and ``reached``."""
    _VALUES = None

    _REDUCE = staticmethod(_segment_sums)                                 # what is made of a fact's edges (EdgeMask: their maximum)

    def _fact_sums(self, inverse_offset=None, who="fact_grad"):
        """(row, fact, sum) of the per-edge values under RDigraph.fact_mask's grouping rule: Saliency.fact_grad states it."""
        rd, values = self.digraph, getattr(self, self._VALUES)
        if _has_times(rd):
            return self._timed_fact_sums(inverse_offset, who)
        E, _ = _check_static_digraph(rd, who)
        if inverse_offset is not None:
            raise ValueError("%s: inverse_offset is for temporal r-digraphs; a static one knows its inverses (r + n_rel)" % who)
        n_rel, dev = int(rd.n_rel), rd.edges.device
        e = rd.edges.long()
        e = e[e[:, 3] != 2 * n_rel]
        if e.shape[0] == 0:
            return (torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros((0, 3), dtype=torch.int64, device=dev),
                    torch.zeros(0, dtype=torch.float32, device=dev))
        inv = e[:, 3] >= n_rel
        h, r, t = torch.where(inv, e[:, 4], e[:, 2]), torch.where(inv, e[:, 3] - n_rel, e[:, 3]), torch.where(inv, e[:, 2], e[:, 4])
        n_key = int(max(h.max(), t.max())) + 1
        key = ((e[:, 0] * n_key + h) * n_rel + r) * n_key + t
        key, order = torch.sort(key, stable=True)                         # copies of a fact in edge order: a fixed order of the sum
        keys, group = torch.unique_consecutive(key, return_inverse=True)
        grad = self._REDUCE(values[rd.edges[:, 3].long() != 2 * n_rel][order], group, keys.numel())
        t_, rest = keys % n_key, keys // n_key
        r_, rest = rest % n_rel, rest // n_rel
        return rest // n_key, torch.stack([rest % n_key, r_, t_], 1), grad

    def _timed_fact_sums(self, inverse_offset, who):
        """_fact_sums of a temporal interpolation or extrapolation digraph."""
        rd, values = self.digraph, getattr(self, self._VALUES)
        xtr = _is_extrapolation(rd)
        (_check_extrapolation_digraph if xtr else _check_temporal_digraph)(rd, who)
        n_rel, dev, m = int(rd.n_rel), rd.edges.device, inverse_offset
        if m is not None and (isinstance(m, (bool, np.bool_)) or not isinstance(m, (int, np.integer)) or m < 1 or 2 * m > n_rel):
            raise ValueError("%s: inverse_offset must be an integer m with 1 <= m and 2 m <= n_rel = %d, relation r's inverse being r + m "
                             "below m and r - m from there on (got %r)" % (who, n_rel, m))
        e, tm = rd.edges.long(), rd.time.long().to(dev)
        fact = e[:, 3] != n_rel                                           # the identity is no fact
        if xtr:
            fact = fact & (rd.data_row.to(dev) >= 0)                      # ... and a self-loop has no data row
        e, tm = e[fact], tm[fact]
        if e.shape[0] == 0:
            return (torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros((0, 4), dtype=torch.int64, device=dev),
                    torch.zeros(0, dtype=torch.float32, device=dev))
        h, r, t = e[:, 2], e[:, 3], e[:, 4]
        if m is not None:
            inv = (r >= int(m)) & (r < 2 * int(m))
            h, r, t = torch.where(inv, e[:, 4], h), torch.where(inv, r - int(m), r), torch.where(inv, e[:, 2], t)
        n_key, n_r, n_t = int(max(h.max(), t.max())) + 1, n_rel + 1, int(tm.max()) + 1
        key = (((e[:, 0] * n_key + h) * n_r + r) * n_key + t) * n_t + tm
        key, order = torch.sort(key, stable=True)                         # copies of a fact in edge order: a fixed order of the sum
        keys, group = torch.unique_consecutive(key, return_inverse=True)
        grad = _segment_sums(values[fact][order], group, keys.numel())
        tm_, rest = keys % n_t, keys // n_t
        t_, rest = rest % n_key, rest // n_key
        r_, rest = rest % n_r, rest // n_r
        return rest // n_key, torch.stack([rest % n_key, r_, t_, tm_], 1), grad

    def top(self, k):
        """The k facts of every row with the largest |value| (fact_grad / fact_attr), largest first, ties in (h, r, t) order: (fact int64 [B, k, 3],
        grad float32 [B, k], count int64 [B]); -1 and 0 where the row has fewer than k facts.  On a temporal digraph fact is
        [B, k, 4] = (h, r, t, time id | day), ties in (h, r, t, time) order."""
        _check_count(k, "top", "k")
        k, B, dev = int(k), self.score.numel(), self.score.device
        row, fact, grad = self._fact_sums()
        order = torch.sort(-grad.abs(), stable=True).indices
        order = order[torch.sort(row[order], stable=True).indices]        # by row, inside a row by |grad| descending
        row, fact, grad = row[order], fact[order], grad[order]
        total = torch.bincount(row, minlength=B)
        rank = torch.arange(row.numel(), device=dev) - (torch.cumsum(total, 0) - total)[row]
        sel = rank < k
        out_f = torch.full((B, k, fact.shape[1]), -1, dtype=torch.int64, device=dev)
        out_g = torch.zeros((B, k), dtype=torch.float32, device=dev)
        out_f[row[sel], rank[sel]] = fact[sel]
        out_g[row[sel], rank[sel]] = grad[sel]
        return out_f, out_g, total.clamp(max=k)

    def format(self, id2rel=None, k=3):
        """One line per row: the score (``x``: o is not reached), then the row's ``k`` facts of largest |value| as (h, relation, t)
        with their gradient (Saliency) or attribution (Attribution) - (h, relation, t, @time) on a temporal digraph; ``id2rel`` names
        the relations."""
        fact, grad, count = (t.cpu().tolist() for t in self.top(k))
        sc, ok = self.score.cpu().tolist(), self.reached.cpu().tolist()
        name = lambda r: str(id2rel[r]) if id2rel is not None else "r%d" % r
        cell = lambda f: "(%d, %s, %d, @%d)" % (f[0], name(f[1]), f[2], f[3]) if len(f) == 4 else "(%d, %s, %d)" % (f[0], name(f[1]), f[2])
        return ["row %d: score %s  %s" % (b, "%.4f" % sc[b] if ok[b] else "x",
                                         "  ".join("%s %+.4f" % (cell(f), g) for f, g in zip(fact[b][:count[b]], grad[b])))
                for b in range(len(sc))]


@dataclass
class Saliency(_FactSums):
    """The gradient of an answer's score with respect to a gate on every edge of its r-digraph (RDigraph.saliency).  Tensors on the
    digraph's device.

    score      float32 [B]  the model's score of o on the kept digraph, exactly 0 where o is not reached     (as Rescore's)
    reached    bool [B]     o has a length-L walk from s through kept edges
    live       bool [E]     the edge is kept and its head is visited at hop - 1; only live edges carry messages
    alpha      float32 [E]  the attention on the kept digraph, 0 for dead edges
    edge_grad  float32 [E]  d score(o of the edge's row) / d g_e at g == 1, g_e multiplying the edge's message; exactly 0 for dead
                            edges and for the rows that are not reached
    digraph    RDigraph     the digraph the edges are those of
    """
    score: torch.Tensor
    reached: torch.Tensor
    live: torch.Tensor
    alpha: torch.Tensor
    edge_grad: torch.Tensor
    digraph: RDigraph
    _VALUES = "edge_grad"

    def fact_grad(self, inverse_offset=None):
        """(row int64 [F], fact int64 [F, 3] = (h, r, t) with r < n_rel, grad float32 [F]) ordered by (row, h, r, t): ``edge_grad``
        summed over all copies of a base fact in its row - the edge (h, r, t) and its twin (t, r + n_rel, h), at every hop; the
        identity relation 2 * n_rel is no fact.  RDigraph.fact_mask's grouping rule: to first order the score of the row changes by
        -grad when the fact is deleted.  ``inverse_offset`` is fact_mask's: a static digraph knows its inverses and takes None.

        On a temporal digraph (interpolation or extrapolation) fact is int64 [F, 4] = (h, r, t, time id | day), ordered by (row, h, r,
        t, time), grouped under fact_mask's temporal rule: every copy of a quadruple in its row at every hop; the identity relation
        n_rel is no fact, and neither is an extrapolation self-loop (data_row < 0).  With ``inverse_offset`` = m an edge with
        m <= r < 2 m counts as (t, r - m, h, time), so that for every returned fact with r < m (every fact when m is None) grad is
        the sum of ``edge_grad`` over fact_mask([fact], rows=[row], inverse_offset=m)."""
        return self._fact_sums(inverse_offset, "fact_grad")

    def data_row_grad(self):
        """Extrapolation digraphs only: (row int64 [F], data_row int64 [F], grad float32 [F]) ordered by (row, data_row): ``edge_grad``
        summed over the edges of a data row in its row, at every hop - RDigraph.data_row_mask's grouping, the exact identity of a
        past fact; self-loops (data_row < 0) are left out."""
        rd = self.digraph
        _check_extrapolation_digraph(rd, "data_row_grad")
        dev = rd.edges.device
        dr = rd.data_row.to(dev).long()
        fact = dr >= 0
        row, dr = rd.edges[:, 0].long()[fact], dr[fact]
        if dr.numel() == 0:
            return (torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev),
                    torch.zeros(0, dtype=torch.float32, device=dev))
        n_key = int(dr.max()) + 1
        key, order = torch.sort(row * n_key + dr, stable=True)
        keys, group = torch.unique_consecutive(key, return_inverse=True)
        return keys // n_key, keys % n_key, _segment_sums(self.edge_grad[fact][order], group, keys.numel())

    def deletion_estimate(self, mask):
        """float32 [B]: score - the sum of ``edge_grad`` over the live edges of ``mask`` (bool or uint8 [E]) per row, the first-order
        estimate of ``rescore(keep=~mask).score``: every gate of the mask taken from 1 to 0 along the tangent."""
        rd = self.digraph
        E = self.edge_grad.numel()
        mask = _check_keep("deletion_estimate", mask, E, self.edge_grad.device)
        if mask is None:
            raise ValueError("deletion_estimate: mask must be bool or uint8 [%d], one per edge (got None)" % E)
        gone = mask.bool() & self.live
        return self.score - _segment_sums(torch.where(gone, self.edge_grad, torch.zeros_like(self.edge_grad)), rd.edges[:, 0].long(),
                                          self.score.numel())


@dataclass
class Attribution(_FactSums):
    """Integrated gradients of an answer's score along the straight path of gates from a baseline to a target
    (RDigraph.integrated_gradients): per-edge attributions that add up to score - baseline_score per row, up to the quadrature error
    ``residual``.  Tensors on the digraph's device.

    score           float32 [B]  the model's score of o at the target gates, exactly 0 where o is not reached
    baseline_score  float32 [B]  ... at the baseline gates
    edge_attr       float32 [E]  (target - baseline) * the midpoint-rule mean of d score / d g_e along the path; exactly 0 for dead
                                 edges, for the rows that are not reached and where target == baseline
    residual        float32 [B]  score - baseline_score - the sum of the row's edge_attr (added in a fixed order): what ``steps``
                                 midpoints leave of the path integral
    reached         bool [B]     o has a length-L walk from s through kept edges: structural, whatever the gates
    live            bool [E]     the edge is kept and its head is visited at hop - 1: structural as well, a gate of 0 disconnects nothing
    steps           int          the quadrature steps
    digraph         RDigraph     the digraph the edges are those of
    """
    score: torch.Tensor
    baseline_score: torch.Tensor
    edge_attr: torch.Tensor
    residual: torch.Tensor
    reached: torch.Tensor
    live: torch.Tensor
    steps: int
    digraph: RDigraph
    _VALUES = "edge_attr"

    def fact_attr(self, inverse_offset=None):
        """(row int64 [F], fact int64 [F, 3] = (h, r, t) with r < n_rel, attr float32 [F]) ordered by (row, h, r, t): ``edge_attr``
        summed over all copies of a base fact in its row, Saliency.fact_grad's grouping (the identity relation is no fact, so with the
        default baseline a row's fact_attr add up to the row's edge_attr).  ``top(k)`` and ``format(id2rel)`` rank by it."""
        return self._fact_sums(inverse_offset, "fact_attr")


@dataclass
class EdgeMask(_FactSums):
    """A learned edge mask of an r-digraph (RDigraph.learn_mask): per row the gates of the replica (the lambda) the selection rule
    took.  Tensors on the digraph's device; R = len(lambdas).

    gate            float32 [E]     the soft gates of the row's replica: 1 at kept self-loops, 0 at edges that are not kept
    keep            bool [E]        the mask: gate > 0.5 on the free edges, the kept self-loops, nothing else
    score           float32 [B]     the score at ``gate`` (the soft score of the row's replica)
    hard_score      float32 [B]     ... at the gates rounded to 0 / 1 (the other edges gated off, their attention left as it was)
    kept_score      float32 [B]     ... of ``rescore(keep=keep)``: the other facts deleted
    target          float32 [B]     the score at gate 1, exactly 0 where o is not reached
    baseline_score  float32 [B]     the score with every free edge at gate 0
    size            int64 [B]       free edges of the row with gate > 0.5
    n_free          int64 [B]       free edges of the row
    replica         int64 [B]       the replica the row took
    lambdas         float32 [R]     the size weights, one per replica
    history         namespace       per iteration i and replica: ``deviation`` float32 [iterations, R, B] = (score - target) / scale
                                    at the gates iteration i starts from, ``size`` float32 and ``count`` int32 [iterations, R, B] = the
                                    sum of the free gates it ends with and how many are above 0.5
    reached         bool [B]        o has a length-L walk from s through kept edges: structural, whatever the gates
    live            bool [E]        the edge is kept and its head is visited at hop - 1: structural as well
    digraph         RDigraph        the digraph the edges are those of
    replica_gate, replica_score, replica_hard_score, replica_size   float32 [R, E], float32 [R, B], float32 [R, B], int64 [R, B]: what
                                    the selection saw of every replica

    A TIED mask (RDigraph.learn_tied_mask; None otherwise) also carries
    tie             "fact", "relation" or the label tensor
    group           int64 [E]       the group whose gate the edge reads, -1 where it is not tied (not free)
    group_row       int64 [G]       the row of every group; groups are ordered by (row, key)
    group_key       int64 [G, c]    "fact": (h, r, t) with r < n_rel; "relation": (hop, rel); labels: (label,)
    group_gate      float32 [G]     the group's gate in its row's replica: ``gate`` at every member edge, bit for bit
    n_groups        int64 [B]       groups of the row
    and there ``size``, ``replica_size`` and ``history.size`` / ``history.count`` count GROUPS (facts under "fact"), while ``n_free``
    keeps its meaning: the row's free edges.
    """
    gate: torch.Tensor
    keep: torch.Tensor
    score: torch.Tensor
    hard_score: torch.Tensor
    kept_score: torch.Tensor
    target: torch.Tensor
    baseline_score: torch.Tensor
    size: torch.Tensor
    n_free: torch.Tensor
    replica: torch.Tensor
    lambdas: torch.Tensor
    history: types.SimpleNamespace
    reached: torch.Tensor
    live: torch.Tensor
    digraph: RDigraph
    replica_gate: torch.Tensor = None
    replica_score: torch.Tensor = None
    replica_hard_score: torch.Tensor = None
    replica_size: torch.Tensor = None
    tie: object = None
    group: torch.Tensor = None
    group_row: torch.Tensor = None
    group_key: torch.Tensor = None
    group_gate: torch.Tensor = None
    n_groups: torch.Tensor = None
    _VALUES = "gate"
    _REDUCE = staticmethod(_segment_max)

    def groups(self):
        """(row int64 [G], key int64 [G, c], gate float32 [G]) of a tied mask, ordered by (row, key): every group with the gate its row's
        replica gave it.  Under tie="fact" this is ``fact_gate()`` with no maximum to take: all copies of a fact hold one gate."""
        if self.group_gate is None:
            raise ValueError("groups: the mask is not tied (learn_tied_mask / learn_mask(tie=) make tied ones)")
        return self.group_row, self.group_key, self.group_gate

    def format_groups(self, id2rel=None, k=3):
        """One line per row: its ``k`` groups of the largest gate, largest first, ties in key order - ``hop1 r3 0.98`` under
        tie="relation" (a soft rule body: which relations, at which hop, carry the answer), ``(h, r3, t) 0.98`` under "fact", the
        label otherwise; ``id2rel`` names the relations."""
        _check_count(k, "format_groups", "k")
        row, key, gate = (t.cpu() for t in self.groups())
        name = lambda r: str(id2rel[r]) if id2rel is not None else "r%d" % r
        if isinstance(self.tie, str) and self.tie == "relation":
            cell = lambda q: "hop%d %s" % (q[0], name(q[1]))
        elif isinstance(self.tie, str) and self.tie == "fact":
            cell = lambda q: "(%d, %s, %d)" % (q[0], name(q[1]), q[2])
        else:
            cell = lambda q: " ".join("%d" % x for x in q)
        order = torch.sort(-gate, stable=True).indices
        order = order[torch.sort(row[order], stable=True).indices]            # by row, inside a row by gate descending
        lines = [[] for _ in range(self.score.numel())]
        for b, q, g in zip(row[order].tolist(), key[order].tolist(), gate[order].tolist()):
            if len(lines[b]) < int(k):
                lines[b].append("%s %.2f" % (cell(q), g))
        return ["row %d: %s" % (b, "  ".join(cells)) for b, cells in enumerate(lines)]

    def fact_gate(self):
        """(row int64 [F], fact int64 [F, 3] = (h, r, t) with r < n_rel, gate float32 [F]) ordered by (row, h, r, t): the largest
        ``gate`` over all copies of a base fact in its row, Saliency.fact_grad's grouping (the identity relation is no fact): a fact
        is in the mask as soon as one of its edges is.  ``top(k)`` and ``format(id2rel)`` rank by it."""
        return self._fact_sums(None, "fact_gate")

    def sufficiency_gap(self):
        """float32 [B]: target - kept_score, what the mask's facts alone fail to reproduce (0: they are sufficient)."""
        return self.target - self.kept_score


def _digraph_family(rd):
    return "an extrapolation" if _is_extrapolation(rd) else "a temporal interpolation" if _has_times(rd) else "a static"


def _saliency_timed(rd, model, keep, mode, n_dir):
    """RDigraph.saliency of a temporal interpolation (n_dir = 3) or extrapolation (n_dir = 1) digraph: the rescore with a tape, then
    the hops backwards.  Neither model has a GRU, so a hop's new state is act(agg) and nothing else carries the old one."""
    from .temporal import eval_semantics
    tape = []
    rs = (rescore_temporal if n_dir == 3 else rescore_extrapolation)(rd, model, keep, mode, "saliency", tape)
    dev, L = rd.edges.device, int(rd.n_hops)
    d, a = model.hidden_dim, model.attn_dim
    edge_grad = torch.zeros(rd.edges.shape[0], dtype=torch.float32, device=dev)
    out = lambda: Saliency(score=rs.score, reached=rs.reached, live=rs.live, alpha=rs.alpha, edge_grad=edge_grad, digraph=rd)
    if len(tape) < L:                                                     # no row reaches its answer: nothing depends on any edge
        return out()
    g_state = None                                                        # d (sum of the scores) / d (the hop's new state) [n_dst, d]
    for t in reversed(tape):
        last, first = t["l"] == L, t["l"] == 1
        if last:                                                          # every hop-L node is its row's answer: the classifier's row
            g_state = model.linear_classifier.weight.detach().reshape(1, d).expand(t["agg"].shape[0], d)
        # ---- through the activation, on the taped sums (eval semantics: no dropout; it has no parameters)
        with torch.enable_grad(), eval_semantics(model):
            agg = t["agg"].detach().requires_grad_(True)
            g_agg, = torch.autograd.grad([model.act(agg[:, :d])], [agg], [g_state.contiguous()])
        # ---- the edge-list layer's adjoint, in HIP
        gate_grad, g_dir, g_a_s = engine.digraph_tlayer_bwd(
            t["dst_ptr"], t["src"], t["rel"], t["row_of"], t["hidden"], t["rela"], t["time_tab"], d, t["a_s"], t["a_r"], t["a_q"],
            t["w_alpha"].detach(), t["b_alpha"], a, g_agg.contiguous(), edge_time=t["edge_time"], q_time=t["q_time"], n_dir=n_dir,
            want_state=not first)
        edge_grad[t["at"]] = gate_grad
        if not first:
            # ---- back through the direction linears (row n_dir s + dir of the directed state is W_dir state[s]) and the attention
            # projection: plain products with the detached weights
            with torch.no_grad():
                n_old = t["a_s"].shape[0]
                g_state = g_dir[:, :d].reshape(n_old, n_dir * d) @ t["w_dir"].detach() + g_a_s[:, :a] @ t["w_s"].detach()
    return out()


def saliency(rd, model, keep=None, mode="test", gate=None):
    """RDigraph.saliency (see there).  The driver is chosen by the model's class: a temporal.T_RED_GNN walks a temporal interpolation
    digraph, an extrapolation.T_RED_GNN an extrapolation one (_saliency_timed); every other model takes the static path -
    _rescore_static with a tape, then the hops backwards.  With ``gate`` the gated walk (_gated_call) takes over."""
    from .models import gru_step, tall_linear
    if gate is not None:
        return _gated_call(rd, model, keep, mode, gate, "saliency", True)
    from .extrapolation import T_RED_GNN as XModel
    from .temporal import T_RED_GNN as TModel
    if isinstance(model, XModel):
        if not _is_extrapolation(rd):
            raise ValueError("saliency: an extrapolation.T_RED_GNN walks the extrapolation r-digraphs it explained (data_row is set, "
                             "n_time is not); this is %s r-digraph" % _digraph_family(rd))
        return _saliency_timed(rd, model, keep, mode, 1)
    if isinstance(model, TModel):
        if _is_extrapolation(rd) or not _has_times(rd):
            raise ValueError("saliency: a temporal.T_RED_GNN walks the temporal interpolation r-digraphs it explained (time, q_time and "
                             "n_time are set, data_row is not); this is %s r-digraph" % _digraph_family(rd))
        return _saliency_timed(rd, model, keep, mode, 3)
    tape = []
    rs = _rescore_static(rd, model, keep, mode, "saliency", tape)
    dev, L = rd.edges.device, int(rd.n_hops)
    d, a = model.hidden_dim, model.attn_dim
    ld, ap = max(16, _pad4(d)), pad_attn(a)
    edge_grad = torch.zeros(rd.edges.shape[0], dtype=torch.float32, device=dev)
    if len(tape) < L:                                                     # no row reaches its answer: nothing depends on any edge
        return Saliency(score=rs.score, reached=rs.reached, live=rs.live, alpha=rs.alpha, edge_grad=edge_grad, digraph=rd)
    gate = types.SimpleNamespace(**{name: getattr(model.gate, name).detach()
                                    for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
    g_hidden = g_a_s = None                                               # d (sum of the scores) / d (the hop's new state, its projection)
    for t in reversed(tape):
        l = t["l"]
        layer, last, first = model.gnn_layers[l - 1], t["l"] == L, t["l"] == 1
        # ---- the dense step's adjoint: _rescore_static's tall_linear / gru_step branch re-run on the hop's sums, parameters detached
        with torch.enable_grad():
            agg = t["agg"].detach().requires_grad_(True)
            prev = t["hidden"].detach().requires_grad_(not first)        # hop 1 reads the constant 0
            x = layer.act(tall_linear(agg[:, :d], layer.W_h.weight.detach()))
            h0 = torch.zeros((agg.shape[0], d), device=dev)
            h0[t["had"]] = prev[:, :d][t["prev_idx"][t["had"]].long()]
            hid = gru_step(x, h0, gate)
            if last:
                outs, seeds = [tall_linear(hid, model.W_final.weight.detach()).squeeze(-1)], [torch.ones(agg.shape[0], device=dev)]
            else:
                w_s = model.gnn_layers[l].Ws_attn.weight.detach()
                outs = [F.pad(hid, (0, ld - d)) if ld != d else hid, tall_linear(hid, F.pad(w_s, (0, 0, 0, ap - a)) if ap != a else w_s)]
                seeds = [g_hidden, g_a_s]
            grads = torch.autograd.grad(outs, [agg] if first else [agg, prev], seeds)
        # ---- the edge-list layer's, in HIP
        gate_grad, g_hidden, g_a_s = engine.digraph_layer_bwd(
            t["dst_ptr"], t["src"], t["rel"], t["row_of"], t["hidden"], t["rela"], d, t["a_s"], t["a_r"], t["a_q"],
            layer.w_alpha.weight.detach().reshape(-1).contiguous(), layer.w_alpha.bias.detach().contiguous(), a, grads[0].contiguous(),
            want_state=not first)
        edge_grad[t["at"]] = gate_grad
        if not first:
            g_hidden = g_hidden + grads[1]                                # the carry: the state also enters the next GRU step as h0
    return Saliency(score=rs.score, reached=rs.reached, live=rs.live, alpha=rs.alpha, edge_grad=edge_grad, digraph=rd)


# ---- gated walks of a static r-digraph: rescore / saliency at any gate, and integrated gradients ------------------------------------
IG_REP_EDGES = 1 << 20               # default rep_chunk: as many replicas as keep replicas * edges at or under this


def _refuse_timed(rd, model, who):
    """The gated edge-list kernels are static: a temporal or extrapolation digraph or model is a ValueError, before any HIP call."""
    from .extrapolation import T_RED_GNN as XModel
    from .temporal import T_RED_GNN as TModel
    if _has_times(rd) or isinstance(model, (XModel, TModel)):
        raise ValueError("%s: gates need the gated edge-list kernels, and their timed forms are not built; static and inductive models "
                         "and their r-digraphs only (this is %s r-digraph and a %s)" % (who, _digraph_family(rd), type(model).__name__))


def _check_gate(who, name, g, E, device):
    """``g`` as a float32 [E] tensor on ``device``: a tensor or a numpy array of that shape and dtype, every entry finite (ValueError)."""
    if not torch.is_tensor(g):
        g = np.asarray(g)
        if g.dtype != np.float32:
            raise ValueError("%s: %s must be float32 [%d], one per edge (got %s)" % (who, name, E, g.dtype))
        g = torch.as_tensor(g)
    if g.dtype != torch.float32 or tuple(g.shape) != (E,):
        raise ValueError("%s: %s must be float32 [%d], one per edge (got %s %s)" % (who, name, E, g.dtype, tuple(g.shape)))
    if not bool(torch.isfinite(g).all()):
        raise ValueError("%s: %s holds a value that is not finite" % (who, name))
    return g.to(device).contiguous()


def _static_hops(S, who):
    """The index of every hop of a static walk, which depends on the kept edges alone - not on the states, the gates or the replicas:
    ([per hop a dict of _hop_index's arrays as the kernels take them], live bool [E], reached bool [B]).  The list ends where no edge
    is live; the source view of a hop (``view``) is added by the first adjoint that needs it."""
    i32 = lambda t: t.to(torch.int32).contiguous()
    live = torch.zeros(S.E, dtype=torch.bool, device=S.dev)
    reached = torch.zeros(S.B, dtype=torch.bool, device=S.dev)
    keys_prev = torch.arange(S.B, device=S.dev) * S.n_ent + S.q_sub           # hop 0: the node (row, s) of every row, sorted
    hops = []
    for l in range(1, S.L + 1):
        at = torch.nonzero((S.hop == l) & S.kept).reshape(-1)
        index = _hop_index(who, l, S.L, at, S.row, S.head, S.tail, keys_prev, S.n_ent, live)
        if index is None:
            break
        at, src, keys, dst_ptr, row_of, prev_idx, had = index
        hops.append(dict(l=l, at=at, src=i32(src), rel=i32(S.rel[at]), dst_ptr=dst_ptr, dst_ptr_host=dst_ptr.cpu().numpy(), row_of=row_of,
                         prev_idx=prev_idx, had=had, n_prev=keys_prev.numel(), n_dst=keys.numel(), view=None))
        if l == S.L:
            reached[row_of] = True
        keys_prev = keys
    return hops, live, reached


def _gated_group(S, rd, model, hops, t, lo, hi, want_grad, check_index=True, gate=None, split_dense=False):
    """One group of n = t.numel() replicas of the static walk, replica k at the gates fmaf(t[k], hi - lo, lo) (``lo`` / ``hi`` float32
    [E] or None for 0 / 1): _rescore_static's hop loop with the replicas' rows stacked, replica k's node j of a hop at row
    k * n_nodes + j - one rg_digraph_layer_fwd_gated launch and one dense step per hop for all of them - and, with ``want_grad``,
    saliency's backward loop on the same stacked rows (rg_digraph_layer_bwd_gated).  Returns (score [n, B], alpha [n, E], grad [n, E]
    or None): the gradient of replica k's scores with respect to its gates.  With n == 1 and gates of 1 every tensor has the bits of
    the ungated walk.  The other gate form, ``gate`` float32 [n, E] (then ``t``, ``lo`` and ``hi`` are None): replica k at the gates
    gate[k], taken as they are (rg_digraph_layer_fwd_gates / rg_digraph_layer_bwd_gates); the walk is the same.  ``split_dense``: the
    dense step's autograd adjoint runs on one replica's rows at a time instead of on the stacked rows.  The HIP launches stay stacked
    and have a replica's bits whatever else they carry; the library GEMMs behind the adjoint do not (their rounding can follow the
    row count), so only with it is replica k's gradient, bit for bit, that of a one-replica call - which learn_mask promises."""
    from .models import gru_step, tall_linear
    n, dev, B, E, L, d, a, ld, ap = (t.numel() if gate is None else gate.shape[0]), S.dev, S.B, S.E, S.L, S.d, S.a, S.ld, S.ap
    score = torch.zeros(n * B, dtype=torch.float32, device=dev)
    alpha = torch.zeros((n, E), dtype=torch.float32, device=dev)
    grad = torch.zeros((n, E), dtype=torch.float32, device=dev) if want_grad else None
    rep = torch.arange(n, device=dev)[:, None]
    w_b = lambda layer: (layer.w_alpha.weight.detach().reshape(-1).contiguous(), layer.w_alpha.bias.detach().contiguous())
    tape = []
    with torch.no_grad():
        tables = model.inference_tables(rd.q_rel.contiguous(), ld, ap)
        hidden = torch.zeros((n * B, ld), device=dev)
        a_s = torch.zeros((n * B, ap), device=dev)                            # hidden == 0 at layer 0
        for h in hops:
            l, at = h["l"], h["at"]
            layer, last = model.gnn_layers[l - 1], l == L
            a_r, a_q, rela_p = (x.contiguous() for x in tables[l - 1])
            # the hop's gates in either form: what follows attn_dim in the forward's and grad_agg in the adjoint's arguments
            if gate is None:
                fwd, bwd = engine.digraph_layer_fwd_gated, engine.digraph_layer_bwd_gated
                g_hop = (t,) + tuple(None if g is None else g[at].contiguous() for g in (lo, hi))
            else:
                fwd, bwd, g_hop = engine.digraph_layer_fwd_gates, engine.digraph_layer_bwd_gates, (gate[:, at].contiguous(),)
            agg, al = fwd(h["dst_ptr"], h["src"], h["rel"], h["row_of"].to(torch.int32).contiguous(), hidden, rela_p, d, a_s, a_r, a_q,
                          *w_b(layer), a, *g_hop, dst_ptr_host=h["dst_ptr_host"], check_index=check_index)
            alpha[:, at] = al.view(n, -1)
            # the GEMM library of the dense step and of its adjoint, chosen here as the model's forward chooses it per layer: torch's
            # choice is one switch per process, and left as the last forward set it the adjoint's last bits followed what had run before.
            # The count is ONE replica's rows, never the stacked ones: a replica of a stacked call must get the library of its own call
            engine.prefer_blas(h["n_dst"])
            # the replicas' rows of the dense step: node j of replica k is row k * n_dst + j, its old state row k * n_prev + prev_idx[j]
            had = h["had"].repeat(n)
            prev_idx = torch.where(h["had"][None, :], h["prev_idx"][None, :] + (rep * h["n_prev"]).to(torch.int32),
                                   h["prev_idx"][None, :]).reshape(-1).contiguous()
            row_of = (h["row_of"][None, :] + rep * B).reshape(-1)
            if want_grad:
                tape.append(dict(h=h, hidden=hidden, a_s=a_s, agg=agg, prev_idx=prev_idx, had=had, a_r=a_r, a_q=a_q, rela=rela_p,
                                 bwd=bwd, g_hop=g_hop))
            if S.fused:                                                       # the dense step of _forward_inference
                node_rows = torch.stack([row_of, torch.zeros_like(row_of)], 1).to(torch.int32).contiguous()
                hidden, a_s = engine.dense_fwd(agg, hidden, prev_idx, d, layer.W_h.weight, model.act_name, model.gate,
                                               Ws_next=None if last else model.gnn_layers[l].Ws_attn.weight, attn_dim=a, ap=ap,
                                               W_final=model.W_final.weight if last else None, nodes=node_rows, n_ent=1,
                                               scores_all=score, precision=model.dense_precision, want_hidden=not last)
            else:                                                             # ... and of _run's ``kept`` branch
                x = layer.act(tall_linear(agg[:, :d], layer.W_h.weight))
                h0 = torch.zeros((agg.shape[0], d), device=dev)
                h0[had] = hidden[:, :d][prev_idx[had].long()]
                hid = gru_step(x, h0, model.gate)
                if last:
                    score[row_of] = tall_linear(hid, model.W_final.weight).squeeze(-1)
                else:
                    w_s = model.gnn_layers[l].Ws_attn.weight
                    a_s = tall_linear(hid, F.pad(w_s, (0, 0, 0, ap - a)) if ap != a else w_s).contiguous()
                    hidden = (F.pad(hid, (0, ld - d)) if ld != d else hid).contiguous()
    score = score.view(n, B)
    if not want_grad or len(hops) < L:                                        # no row reaches its answer: nothing depends on any edge
        return score, alpha, grad
    gru = types.SimpleNamespace(**{name: getattr(model.gate, name).detach()
                                   for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")})
    g_hidden = g_a_s = None                                                   # d (sum of the scores) / d (the hop's new state, its projection)
    for tp in reversed(tape):
        h = tp["h"]
        l = h["l"]
        layer, last, first = model.gnn_layers[l - 1], l == L, l == 1
        engine.prefer_blas(h["n_dst"])                                        # (the hop's own choice again, per replica: a later hop may have moved it)
        # ---- the dense step's adjoint: saliency's, on the stacked rows - or, with ``split_dense``, on one replica's rows at a time
        def dense_adjoint(agg, prev, had, prev_idx, seeds):
            with torch.enable_grad():
                agg = agg.detach().requires_grad_(True)
                prev = prev.detach().requires_grad_(not first)                # hop 1 reads the constant 0
                x = layer.act(tall_linear(agg[:, :d], layer.W_h.weight.detach()))
                h0 = torch.zeros((agg.shape[0], d), device=dev)
                h0[had] = prev[:, :d][prev_idx[had].long()]
                hid = gru_step(x, h0, gru)
                if last:
                    outs, seeds = [tall_linear(hid, model.W_final.weight.detach()).squeeze(-1)], [torch.ones(agg.shape[0], device=dev)]
                else:
                    w_s = model.gnn_layers[l].Ws_attn.weight.detach()
                    outs = [F.pad(hid, (0, ld - d)) if ld != d else hid, tall_linear(hid, F.pad(w_s, (0, 0, 0, ap - a)) if ap != a else w_s)]
                return torch.autograd.grad(outs, [agg] if first else [agg, prev], seeds)

        if split_dense and n > 1:
            n_d, n_p = h["n_dst"], h["n_prev"]
            parts = [dense_adjoint(tp["agg"][k * n_d:(k + 1) * n_d], tp["hidden"][k * n_p:(k + 1) * n_p], h["had"], h["prev_idx"],
                                   None if last else [g_hidden[k * n_d:(k + 1) * n_d], g_a_s[k * n_d:(k + 1) * n_d]]) for k in range(n)]
            grads = [torch.cat([p[i] for p in parts], 0) for i in range(len(parts[0]))]
        else:
            grads = dense_adjoint(tp["agg"], tp["hidden"], tp["had"], tp["prev_idx"], None if last else [g_hidden, g_a_s])
        # ---- the edge-list layer's, in HIP, on the hop's source view (built once per hop, whatever the gates and the replicas)
        if h["view"] is None:
            h["view"] = engine.digraph_source_view(h["dst_ptr"], h["src"], h["n_prev"])
        gate_grad, g_hidden, g_a_s = tp["bwd"](
            h["dst_ptr"], h["src"], h["rel"], h["row_of"].to(torch.int32).contiguous(), tp["hidden"], tp["rela"], d, tp["a_s"], tp["a_r"],
            tp["a_q"], *w_b(layer), a, grads[0].contiguous(), *tp["g_hop"], want_state=not first, view=h["view"],
            check_index=check_index)
        grad[:, h["at"]] = gate_grad.view(n, -1)
        if not first:
            g_hidden = g_hidden + grads[1]                                    # the carry: the state also enters the next GRU step as h0
    return score, alpha, grad


def _gated_setup(rd, model, keep, mode, who, gates, tie=None):
    """The refusals and checks of a gated call, in the order that lets a host without a device reach them: the family, the digraph's
    tensors, then ``gates`` - {name: float32 [E] or None} - and the labels of a tensor ``tie`` (learn_mask), which need E, and only
    then _static_setup, which needs the device.  Returns (S, gates on the device)."""
    _refuse_timed(rd, model, who)
    E, _ = _check_static_digraph(rd, who)
    gates = {name: None if g is None else _check_gate(who, name, g, E, rd.edges.device) for name, g in gates.items()}
    _check_tie_labels(who, tie, E)
    S = _static_setup(rd, model, keep, mode, who)
    S.q_sub = rd.q_sub
    return S, gates


def _gated_call(rd, model, keep, mode, gate, who, want_grad):
    """RDigraph.rescore / saliency with ``gate``: one replica at lo == hi == gate, so the kernels' gate is that value exactly."""
    S, g = _gated_setup(rd, model, keep, mode, who, dict(gate=gate))
    hops, live, reached = _static_hops(S, who)
    t = torch.ones(1, dtype=torch.float32, device=S.dev)
    score, alpha, grad = _gated_group(S, rd, model, hops, t, g["gate"], g["gate"], want_grad)
    if not want_grad:
        return Rescore(score=score[0], reached=reached, live=live, alpha=alpha[0])
    return Saliency(score=score[0], reached=reached, live=live, alpha=alpha[0], edge_grad=grad[0], digraph=rd)


def integrated_gradients(rd, model, steps=16, keep=None, baseline=None, target=None, rep_chunk=None, mode="test"):
    """RDigraph.integrated_gradients (see there)."""
    who = "integrated_gradients"
    _refuse_timed(rd, model, who)
    _check_count(steps, who, "steps")
    if rep_chunk is not None:
        _check_count(rep_chunk, who, "rep_chunk")
    S, g = _gated_setup(rd, model, keep, mode, who, dict(baseline=baseline, target=target))
    steps, E, B, dev = int(steps), S.E, S.B, S.dev
    lo = (S.rel == 2 * int(rd.n_rel)).to(torch.float32) if g["baseline"] is None else g["baseline"]     # self-loops are not facts
    hi = torch.ones(E, dtype=torch.float32, device=dev) if g["target"] is None else g["target"]
    hops, live, reached = _static_hops(S, who)                                # the index: once, whatever the gates
    ends = torch.tensor([0.0, 1.0], dtype=torch.float32, device=dev)          # the two ends of the path in one call, no adjoint
    score, _, _ = _gated_group(S, rd, model, hops, ends, lo, hi, False)
    diff = hi - lo
    weight = diff * (1.0 / steps)
    edge_attr = torch.zeros(E, dtype=torch.float32, device=dev)
    n_group = max(1, min(steps, IG_REP_EDGES // max(E, 1))) if rep_chunk is None else int(rep_chunk)
    for k0 in range(0, steps, n_group):
        k = torch.arange(k0, min(k0 + n_group, steps), dtype=torch.float64, device=dev)
        t = ((k + 0.5) / steps).to(torch.float32)                             # the midpoint rule
        _, _, grad = _gated_group(S, rd, model, hops, t, lo, hi, True, check_index=False)
        for j in range(t.numel()):                                            # k ascending: a fixed order of the sum
            edge_attr += weight * grad[j]
    edge_attr = torch.where(diff != 0, edge_attr, torch.zeros_like(edge_attr))
    residual = score[1] - score[0] - _segment_sums(edge_attr, S.row, B)
    return Attribution(score=score[1], baseline_score=score[0], edge_attr=edge_attr, residual=residual, reached=reached, live=live,
                       steps=steps, digraph=rd)


MASK_SPLIT_DENSE = True              # learn_mask: the dense step's autograd adjoint per replica (a replica's gates are then, bit for bit,
#                                      those of a one-replica call); False: on the stacked rows, as integrated gradients runs it - about
#                                      3.6 x faster per iteration at DESIGN 5's sizes, the gradients equal up to the last bits


def _check_mask_args(who, lambdas, entropy, iterations, lr, theta0, tol):
    """The host checks of learn_mask's own arguments (ValueError naming the argument); returns the lambdas as a float32 array."""
    try:
        lam = np.asarray(list(lambdas), dtype=np.float64)
    except (TypeError, ValueError):
        lam = None
    if lam is None or lam.ndim != 1 or lam.size < 1 or not np.isfinite(lam).all() or (lam < 0).any():
        raise ValueError("%s: lambdas must be a non-empty sequence of finite values >= 0 (got %r)" % (who, lambdas))
    real = lambda x: isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, (bool, np.bool_)) and np.isfinite(x)
    if not real(entropy) or entropy < 0:
        raise ValueError("%s: entropy must be a finite value >= 0 (got %r)" % (who, entropy))
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError("%s: iterations must be a count >= 0 (got %r)" % (who, iterations))
    if not real(lr) or lr <= 0:
        raise ValueError("%s: lr must be a finite value > 0 (got %r)" % (who, lr))
    if not real(tol) or tol < 0:
        raise ValueError("%s: tol must be a finite value >= 0 (got %r)" % (who, tol))
    if not real(theta0):
        raise ValueError("%s: theta0 must be finite (got %r)" % (who, theta0))
    return lam.astype(np.float32)


def mask_selection(hard_score, size, target, scale, tol):
    """learn_mask's selection rule: int64 [B], per row the replica with the fewest gates above 0.5 (``size`` int64 [R, B]) among those
    with |hard_score - target| <= tol * scale (``hard_score`` float32 [R, B]), or, where there is none, the one of the smallest
    deviation; ties to the lower replica."""
    R = hard_score.shape[0]
    k = torch.arange(R, device=hard_score.device)[:, None]
    dev_h = (hard_score - target[None, :]).abs()
    ok = dev_h <= tol * scale[None, :]
    by_size = torch.where(ok, size * R + k, torch.full_like(size, torch.iinfo(torch.int64).max)).min(0).values % R
    by_dev = torch.where(dev_h == dev_h.min(0, keepdim=True).values, k, R).min(0).values
    return torch.where(ok.any(0), by_size, by_dev)


MASK_TIES = ("fact", "relation")


def _check_tie(who, tie):
    """The kind of ``tie``, checked with learn_mask's own arguments: None, one of MASK_TIES, or a tensor / numpy array of labels
    (whose dtype and shape need E: _check_tie_labels)."""
    if tie is None or torch.is_tensor(tie) or isinstance(tie, np.ndarray) or (isinstance(tie, str) and tie in MASK_TIES):
        return
    raise ValueError('%s: tie must be None, "fact", "relation" or an int64 tensor or array [E] of labels, one per edge (got %r)' % (who, tie))


def _check_tie_labels(who, tie, E):
    """A tensor ``tie``: int64 [E] (ValueError); the named ties and None pass."""
    if tie is None or isinstance(tie, str):
        return
    dtype = tie.dtype
    if dtype not in (torch.int64, np.dtype(np.int64)) or tuple(tie.shape) != (E,):
        raise ValueError("%s: tie must be int64 [%d], one label per edge (got %s %s)" % (who, E, dtype, tuple(tie.shape)))


def mask_groups(rd, tie, free):
    """The groups of tied edges of learn_mask(tie=): which of the edges ``free`` (bool [E]) share one gate.  Pure torch on the digraph's
    device, CPU included.  ``tie``:

        "fact"      the key is (h, r, t) with an inverse edge (t, r + n_rel, h) folded back on its fact: RDigraph.fact_mask's rule and
                    Saliency.fact_grad's grouping; a self-loop (relation 2 * n_rel) is no fact and is never tied
        "relation"  the key is (hop, rel), rel as the edge carries it (an inverse is a relation of its own): a soft rule body per row
        int64 [E]   a tensor or numpy array of labels >= 0 on the free edges: the key is (label,)

    Groups never span rows; they are ordered by (row, key ascending) and a group's members by ascending edge position.  Returns a
    namespace: ``group_of`` int32 [E] (-1: not tied), ``grp_ptr`` int32 [G + 1] with its host copy ``grp_ptr_host`` (numpy) and
    ``member`` int32 [M] as engine.mask_tie_grad takes them, ``row_ptr`` int64 [B + 1] the rows' group ranges, ``group_row`` int64 [G],
    ``group_key`` int64 [G, c] and ``n_groups`` = G.  A tie of another kind, labels of a wrong dtype or shape or a negative label on
    a free edge: ValueError("learn_mask: tie ...")."""
    who = "learn_mask"
    _check_tie(who, tie)
    if tie is None:
        raise ValueError("%s: tie None ties nothing: there are no groups" % who)
    E, B = _check_static_digraph(rd, who)
    _check_tie_labels(who, tie, E)
    dev = rd.edges.device
    free = (free if torch.is_tensor(free) else torch.as_tensor(np.asarray(free))).to(dev)
    if free.dtype not in (torch.bool, torch.uint8) or tuple(free.shape) != (E,):
        raise ValueError("%s: free must be bool [%d], one per edge (got %s %s)" % (who, E, free.dtype, tuple(free.shape)))
    free, e, n_rel = free.bool(), rd.edges.long(), int(rd.n_rel)
    if isinstance(tie, str) and tie == "fact":
        free = free & (e[:, 3] != 2 * n_rel)
        inv = e[:, 3] >= n_rel
        cols = [torch.where(inv, e[:, 4], e[:, 2]), torch.where(inv, e[:, 3] - n_rel, e[:, 3]), torch.where(inv, e[:, 2], e[:, 4])]
    elif isinstance(tie, str):
        cols = [e[:, 1], e[:, 3]]
    else:
        label = (tie.detach() if torch.is_tensor(tie) else torch.as_tensor(tie)).to(dev)
        if bool((label[free] < 0).any()):
            raise ValueError("%s: tie holds a negative label on a free edge" % who)
        cols = [label]
    at = torch.nonzero(free).reshape(-1)
    keys = torch.stack([e[:, 0]] + cols, 1)[at]
    if at.numel():
        keys, inverse = torch.unique(keys, dim=0, return_inverse=True)        # sorted by (row, key)
    else:
        inverse = at
    G = keys.shape[0]
    member = at[torch.sort(inverse, stable=True).indices].to(torch.int32)     # a group's members in edge order
    grp_ptr = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    grp_ptr[1:] = torch.cumsum(torch.bincount(inverse, minlength=G), 0)
    grp_ptr = grp_ptr.to(torch.int32)
    group_of = torch.full((E,), -1, dtype=torch.int32, device=dev)
    group_of[at] = inverse.to(torch.int32)
    row_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(torch.bincount(keys[:, 0], minlength=B)[:B], 0)
    return types.SimpleNamespace(group_of=group_of, grp_ptr=grp_ptr, grp_ptr_host=grp_ptr.cpu().numpy(), member=member.contiguous(),
                                 row_ptr=row_ptr, group_row=keys[:, 0].contiguous(), group_key=keys[:, 1:].contiguous(), n_groups=G)


def learn_mask(rd, model, lambdas=(0.01, 0.03, 0.1, 0.3, 1.0), entropy=0.0, iterations=100, lr=0.05, theta0=2.0, tol=0.05, keep=None,
               mode="test", tie=None):
    """RDigraph.learn_mask, and with ``tie`` RDigraph.learn_tied_mask (see there)."""
    who = "learn_mask"
    lam = _check_mask_args(who, lambdas, entropy, iterations, lr, theta0, tol)
    _check_tie(who, tie)
    if tie is not None:
        return _learn_tied_mask(who, rd, model, lam, entropy, iterations, lr, theta0, tol, keep, mode, tie)
    S, _ = _gated_setup(rd, model, keep, mode, who, {})
    R, E, B, dev, iterations = lam.size, S.E, S.B, S.dev, int(iterations)
    f32 = dict(dtype=torch.float32, device=dev)
    hops, live, reached = _static_hops(S, who)                                # the index: once, whatever the gates
    fixed = S.kept & (S.rel == 2 * int(rd.n_rel))                             # self-loops are not facts: gate 1 throughout
    free = S.kept & ~fixed
    # ---- the two ends in one two-replica walk, as integrated gradients takes them: the free edges at 0, and every gate at 1
    ends, _, _ = _gated_group(S, rd, model, hops, torch.tensor([0.0, 1.0], **f32), fixed.to(torch.float32), torch.ones(E, **f32), False)
    baseline, target = ends[0], ends[1]
    scale = (target - baseline).abs()
    inv_scale = torch.where((scale > 0) & reached, 1.0 / scale, torch.zeros_like(scale))
    n_free = torch.bincount(S.row[free], minlength=B)[:B]
    inv_n = torch.where(n_free > 0, 1.0 / n_free.to(torch.float32), torch.zeros(B, **f32))
    lam_size, lam_ent = torch.as_tensor(lam).to(dev), torch.full((R,), float(entropy), **f32)
    # ---- the state: a logit and Adam's moments per (replica, edge); the gates the kernels read
    theta, m, v = torch.full((R, E), float(theta0), **f32), torch.zeros((R, E), **f32), torch.zeros((R, E), **f32)
    gate = torch.zeros((R, E), **f32)
    gate[:, free] = float(np.float32(1.0 / (1.0 + np.exp(-np.float64(theta0)))))
    gate[:, fixed] = 1.0
    free_u8 = free.to(torch.uint8).contiguous()
    hist = types.SimpleNamespace(deviation=torch.zeros((iterations, R, B), **f32), size=torch.zeros((iterations, R, B), **f32),
                                 count=torch.zeros((iterations, R, B), dtype=torch.int32, device=dev))
    for it in range(iterations):
        score, _, grad = _gated_group(S, rd, model, hops, None, None, None, True, check_index=False, gate=gate, split_dense=MASK_SPLIT_DENSE)
        hist.deviation[it] = (score - target[None, :]) * inv_scale[None, :]
        _, hist.size[it], hist.count[it] = engine.mask_step(rd.offsets, free_u8, score.contiguous(), target, inv_scale, inv_n, lam_size,
                                                            lam_ent, grad, theta, m, v, it + 1, lr=lr, gate_out=gate)
    # ---- selection: the soft gates and the gates rounded at 0.5 of every replica in one stacked walk
    hard = torch.where(free[None, :], (gate > 0.5).to(torch.float32), gate)
    both, _, _ = _gated_group(S, rd, model, hops, None, None, None, False, check_index=False, gate=torch.cat([gate, hard], 0))
    soft_score, hard_score = both[:R], both[R:]
    size = torch.zeros((R, B), dtype=torch.int64, device=dev).index_add_(1, S.row[free], (gate[:, free] > 0.5).long())
    replica = mask_selection(hard_score, size, target, scale, float(tol))
    rows = torch.arange(B, device=dev)
    gate_sel = gate[replica[S.row], torch.arange(E, device=dev)]
    keep_sel = torch.where(free, gate_sel > 0.5, fixed)
    kept = rescore(rd, model, keep=keep_sel, mode=mode)
    return EdgeMask(gate=gate_sel, keep=keep_sel, score=soft_score[replica, rows], hard_score=hard_score[replica, rows],
                    kept_score=kept.score, target=target, baseline_score=baseline, size=size[replica, rows], n_free=n_free, replica=replica,
                    lambdas=lam_size, history=hist, reached=reached, live=live, digraph=rd, replica_gate=gate, replica_score=soft_score,
                    replica_hard_score=hard_score, replica_size=size)


def _learn_tied_mask(who, rd, model, lam, entropy, iterations, lr, theta0, tol, keep, mode, tie):
    """learn_mask with a tie: the untied driver with the state per (replica, group).  An iteration is the same stacked walk at the
    [R, E] gates, then the chain rule through the tie (rg_mask_tie_grad), rg_mask_step on the group arrays - the rows' group ranges
    for offsets, every group free - and the group gates written back to the edges (rg_mask_tie_gates)."""
    S, _ = _gated_setup(rd, model, keep, mode, who, {}, tie)
    R, E, B, dev, iterations = lam.size, S.E, S.B, S.dev, int(iterations)
    f32 = dict(dtype=torch.float32, device=dev)
    hops, live, reached = _static_hops(S, who)
    fixed = S.kept & (S.rel == 2 * int(rd.n_rel))
    free = S.kept & ~fixed
    T = mask_groups(rd, tie, free)
    G = T.n_groups
    ends, _, _ = _gated_group(S, rd, model, hops, torch.tensor([0.0, 1.0], **f32), fixed.to(torch.float32), torch.ones(E, **f32), False)
    baseline, target = ends[0], ends[1]
    scale = (target - baseline).abs()
    inv_scale = torch.where((scale > 0) & reached, 1.0 / scale, torch.zeros_like(scale))
    n_free = torch.bincount(S.row[free], minlength=B)[:B]
    n_groups = T.row_ptr[1:] - T.row_ptr[:-1]
    inv_n = torch.where(n_groups > 0, 1.0 / n_groups.to(torch.float32), torch.zeros(B, **f32))
    lam_size, lam_ent = torch.as_tensor(lam).to(dev), torch.full((R,), float(entropy), **f32)
    # ---- the state: a logit and Adam's moments per (replica, group), the groups' gates, and the edges' gates the kernels read
    g0 = float(np.float32(1.0 / (1.0 + np.exp(-np.float64(theta0)))))
    theta, m, v = torch.full((R, G), float(theta0), **f32), torch.zeros((R, G), **f32), torch.zeros((R, G), **f32)
    grp_gate = torch.full((R, G), g0, **f32)
    gate = torch.zeros((R, E), **f32)
    gate[:, free] = g0
    gate[:, fixed] = 1.0
    all_free = torch.ones(G, dtype=torch.uint8, device=dev)
    hist = types.SimpleNamespace(deviation=torch.zeros((iterations, R, B), **f32), size=torch.zeros((iterations, R, B), **f32),
                                 count=torch.zeros((iterations, R, B), dtype=torch.int32, device=dev))
    for it in range(iterations):
        score, _, grad = _gated_group(S, rd, model, hops, None, None, None, True, check_index=False, gate=gate, split_dense=MASK_SPLIT_DENSE)
        hist.deviation[it] = (score - target[None, :]) * inv_scale[None, :]
        grp_grad = engine.mask_tie_grad(T.grp_ptr, T.member, grad, G, grp_ptr_host=T.grp_ptr_host)
        _, hist.size[it], hist.count[it] = engine.mask_step(T.row_ptr, all_free, score.contiguous(), target, inv_scale, inv_n, lam_size,
                                                            lam_ent, grp_grad, theta, m, v, it + 1, lr=lr, gate_out=grp_gate)
        engine.mask_tie_gates(T.group_of, grp_gate, gate)
    # ---- selection: as the untied driver's, the size of a replica's mask counted in groups
    hard = torch.where(free[None, :], (gate > 0.5).to(torch.float32), gate)
    both, _, _ = _gated_group(S, rd, model, hops, None, None, None, False, check_index=False, gate=torch.cat([gate, hard], 0))
    soft_score, hard_score = both[:R], both[R:]
    size = torch.zeros((R, B), dtype=torch.int64, device=dev).index_add_(1, T.group_row, (grp_gate > 0.5).long())
    replica = mask_selection(hard_score, size, target, scale, float(tol))
    rows = torch.arange(B, device=dev)
    gate_sel = gate[replica[S.row], torch.arange(E, device=dev)]
    keep_sel = torch.where(free, gate_sel > 0.5, fixed)
    kept = rescore(rd, model, keep=keep_sel, mode=mode)
    return EdgeMask(gate=gate_sel, keep=keep_sel, score=soft_score[replica, rows], hard_score=hard_score[replica, rows],
                    kept_score=kept.score, target=target, baseline_score=baseline, size=size[replica, rows], n_free=n_free, replica=replica,
                    lambdas=lam_size, history=hist, reached=reached, live=live, digraph=rd, replica_gate=gate, replica_score=soft_score,
                    replica_hard_score=hard_score, replica_size=size, tie=tie, group=T.group_of.long(), group_row=T.group_row,
                    group_key=T.group_key, group_gate=grp_gate[replica[T.group_row], torch.arange(G, device=dev)], n_groups=n_groups)


def _fidelity_of(rd, model, k, loops, mode, inverse_offset=None):
    """The Fidelity of a digraph: top_paths(k), then per j the two rescores - without the best j paths' facts, and with them and the
    self-loops ``loops`` (bool [E]) alone."""
    paths = rd.top_paths(int(k))
    cols = {name: [] for name in ("without", "only", "reached_without", "reached_only")}
    for j in range(1, int(k) + 1):
        m = paths.fact_mask(j, inverse_offset=inverse_offset)
        wo, on = rd.rescore(model, keep=~m, mode=mode), rd.rescore(model, keep=m | loops, mode=mode)
        for name, v in (("without", wo.score), ("only", on.score), ("reached_without", wo.reached), ("reached_only", on.reached)):
            cols[name].append(v)
    return Fidelity(score=rd.score, count=paths.count, paths=paths, **{name: torch.stack(v, 1) for name, v in cols.items()})


def fidelity(model, subs, rels, objs=None, k=4, mode="test"):
    """RED_GNN_trans.fidelity (see there)."""
    _check_count(k, "fidelity", "k", engine.PATHS_MAX_K)
    rd = model.explain(subs, rels, objs, mode=mode)
    return _fidelity_of(rd, model, k, rd.edges[:, 3] == 2 * model.n_rel, mode)


def temporal_fidelity(model, batch, objs=None, k=4, inverse_offset=None):
    """temporal.T_RED_GNN.fidelity (see there)."""
    _check_count(k, "fidelity", "k", engine.PATHS_MAX_K)
    if objs is None and "tail" in batch:
        objs = batch["tail"]
    rd = model.explain(batch, objs)
    return _fidelity_of(rd, model, k, rd.edges[:, 3] == model.n_rel, "test", inverse_offset)


def temporal_fidelity_all(model, quads, k=4, batch_size=64, inverse_offset=None):
    """temporal.T_RED_GNN.fidelity_all (see there)."""
    q = np.asarray(quads.detach().cpu().numpy() if torch.is_tensor(quads) else quads)
    if q.ndim != 2 or q.shape[1] != 4 or len(q) == 0 or q.dtype == np.bool_ or not np.issubdtype(q.dtype, np.integer):
        raise ValueError("fidelity_all: quads must be a non-empty integer array [n, 4] = (head, rel, tail, time id) (got %s %s)"
                         % (q.dtype, q.shape))
    _check_count(k, "fidelity_all", "k", engine.PATHS_MAX_K)
    _check_count(batch_size, "fidelity_all", "batch_size")
    parts = []
    for lo in range(0, len(q), int(batch_size)):
        part = q[lo:lo + int(batch_size)]
        parts.append(model.fidelity({"head": part[:, 0], "relation": part[:, 1], "time": part[:, 3]}, part[:, 2], k=int(k),
                                    inverse_offset=inverse_offset))
    return _fidelity_summary(parts, k)


def _fidelity_summary(parts, k):
    """The dict BaseModel.fidelity returns, from the Fidelity of every batch."""
    nec = torch.cat([f.necessity().double().cpu() for f in parts])
    gap = torch.cat([f.sufficiency_gap().double().cpu() for f in parts])
    cut = torch.cat([(f.paths.digraph.reached[:, None] & ~f.reached_without).cpu() for f in parts])
    return dict(n=int(nec.shape[0]), k=int(k), necessity_mean=nec.mean(0).tolist(), necessity_median=nec.median(0).values.tolist(),
                sufficiency_gap_mean=gap.mean(0).tolist(), sufficiency_gap_median=gap.median(0).values.tolist(),
                disconnected=cut.double().mean(0).tolist())


def split_fidelity(base, data="test", k=4, batch=50, max_queries=None):
    """BaseModel.fidelity (see there)."""
    if data not in ("valid", "test"):
        raise ValueError("fidelity: data must be 'valid' or 'test' (got %r)" % (data,))
    _check_count(k, "fidelity", "k", engine.PATHS_MAX_K)
    _check_count(batch, "fidelity", "batch")
    loader = base.loader
    query, answer = (loader.valid_q, loader.valid_a) if data == "valid" else (loader.test_q, loader.test_a)
    n = len(query) if max_queries is None else min(len(query), int(max_queries))
    rows = [(int(query[i][0]), int(query[i][1]), min(int(x) for x in answer[i])) for i in range(n) if len(answer[i])]
    if not rows:
        raise ValueError("fidelity: no queries with an answer in the %s split (n=%d)" % (data, n))
    rows = np.array(rows, dtype=np.int64)
    mode = loader.eval_mode(data) if hasattr(loader, "eval_mode") else data
    parts = []
    for lo in range(0, len(rows), int(batch)):
        part = rows[lo:lo + int(batch)]
        parts.append(base.model.fidelity(part[:, 0], part[:, 1], part[:, 2], k=int(k), mode=mode))
    return _fidelity_summary(parts, k)
