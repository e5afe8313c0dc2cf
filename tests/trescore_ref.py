"""Plain-numpy reference of RDigraph.rescore and RDigraph.fact_mask on a temporal interpolation r-digraph, and the inputs the temporal
fidelity tests share.  TEST INFRASTRUCTURE.

rescore: the temporal forward of tests/temporal_ref.walk (un-hoisted: the direction's Linear applied per edge to h_head + rela[rel] +
time_embed[|dt|]) over an explicit edge list (row, hop, head, rel, tail) with a time id per edge, under a keep mask and with the forward
liveness sweep of tests/rescore_ref.py: a kept hop-l edge carries a message iff its head is a node of hop l - 1, hop 0 being (row, s).
``dtype`` np.float64 is the reference, np.float32 the yardstick of what an fp32 evaluation costs.  Nothing here is taken from the
library: a row's digraph is cut out of the walk's own per-hop edge lists (digraph_of), ordered by (row, hop, tail, walk order).
"""
import numpy as np

from tests import temporal_ref as TR

INVERSE_OFFSET = TR.HAND_N_REL                           # hand_graph writes the inverse of relation r < 3 as r + 3
IDENTITY = 2 * TR.HAND_N_REL                             # ... and the identity as 6 = the model's n_rel


def _find(keys, want):
    if len(keys) == 0:
        return np.zeros(len(want), np.int64), np.zeros(len(want), bool)
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return pos, keys[pos] == want


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def rescore(p, edges, time, heads, rels, q_time, n_ent, n_layer, act, keep=None, shared_tables=False, dtype=np.float64):
    """(score [B], reached bool [B], live bool [E], alpha [E]) of the rows' answers on the kept edges.  ``edges`` int [E, 5] = (row,
    hop, head, rel, tail) with ``time`` int [E]; the hop-L edges of a row share their tail, the row's answer.  ``p``: a state dict of
    temporal.T_RED_GNN (arrays or tensors)."""
    dt_ = np.dtype(dtype)
    g = lambda k: np.asarray(p[k].detach().cpu().numpy() if hasattr(p[k], "detach") else p[k]).astype(dt_)
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    row, hop, head, rel, tail = e.T
    time = np.asarray(time, np.int64)
    heads, rels, q_time = (np.asarray(x, np.int64).reshape(-1) for x in (heads, rels, q_time))
    temb = g("time_embed.weight")
    W = [g("past_linear.weight"), g("now_linear.weight"), g("future_linear.weight")]       # by direction 0 / 1 / 2
    B, E, d = len(heads), len(e), temb.shape[1]
    keep = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    score, reached = np.zeros(B, dt_), np.zeros(B, bool)
    live, alpha = np.zeros(E, bool), np.zeros(E, dt_)
    keys_prev = np.arange(B) * n_ent + heads
    hidden = np.zeros((B, d), dt_)
    actf = TR._ACTS[act]
    for l in range(1, n_layer + 1):
        if shared_tables:
            rela, w1, w2 = g("rela_embed.weight"), g("attention_1.weight"), g("attention_2.weight")
        else:
            rela, w1, w2 = (g("%s.%d.weight" % (name, l - 1)) for name in ("rela_embed_layer", "attention_1_layer", "attention_2_layer"))
        at = np.nonzero((hop == l) & keep)[0]
        src, ok = _find(keys_prev, row[at] * n_ent + head[at])
        at, src = at[ok], src[ok]
        if len(at) == 0:
            return score, reached, live, alpha
        live[at] = True
        keys, dst = np.unique(row[at] * n_ent + tail[at], return_inverse=True)
        dt = time[at] - q_time[row[at]]
        d_of = TR.direction(time[at], q_time[row[at]])
        hs, hr = hidden[src], rela[rel[at]]
        embed = hs + hr + temb[np.abs(dt)]
        msg = np.zeros_like(embed)
        for k in range(3):
            msg[d_of == k] = embed[d_of == k] @ W[k].T
        att_in = np.concatenate([hs, hr, rela[rels[row[at]]]], 1)
        al = _sigmoid(np.maximum(att_in @ w1.T, 0) @ w2.T).astype(dt_)
        alpha[at] = al[:, 0]
        agg = np.zeros((len(keys), d), dt_)
        np.add.at(agg, dst.reshape(-1), al * msg)
        hidden = actf(agg).astype(dt_)
        keys_prev = keys
    rows = keys_prev // n_ent
    assert len(np.unique(rows)) == len(rows), "the hop-L edges of a row must share their tail"
    score[rows] = (hidden @ g("linear_classifier.weight").T + g("linear_classifier.bias"))[:, 0]
    reached[rows] = True
    return score, reached, live, alpha


def twin(h, r, t, tm, m):
    return (t, r + m if r < m else r - m, h, tm)


def fact_mask(edges, time, n_rel, facts, rows=None, inverse_offset=None):
    """bool [E]: edge (row, hop, head, rel, tail) at ``time`` is a quadruple (h, r, t, time id) of its row (``rows[f]``; None: of any
    row) or, with ``inverse_offset`` = m, its twin (t, r + m if r < m else r - m, h, time id); the identity relation ``n_rel`` is never
    marked."""
    want = set()
    for f, (h, r, t, tm) in enumerate(np.asarray(facts, np.int64).reshape(-1, 4).tolist()):
        if r == n_rel:
            continue
        b = -1 if rows is None else int(rows[f])
        want.add((b, h, r, t, tm))
        if inverse_offset is not None:
            want.add((b,) + twin(h, r, t, tm, inverse_offset))
    e = np.asarray(edges, np.int64).reshape(-1, 5).tolist()
    return np.array([rel != n_rel and ((-1 if rows is None else b), h, rel, t, int(tm)) in want
                     for (b, _, h, rel, t), tm in zip(e, np.asarray(time).tolist())], dtype=bool)


def without_quads(quads, facts, inverse_offset=None):
    """``quads`` int [n, 4] without every copy of the quadruples ``facts`` and, with ``inverse_offset``, of their twins."""
    gone = set()
    for h, r, t, tm in np.asarray(facts, np.int64).reshape(-1, 4).tolist():
        gone.add((h, r, t, tm))
        if inverse_offset is not None:
            gone.add(twin(h, r, t, tm, inverse_offset))
    q = np.asarray(quads, np.int64)
    return q[np.array([tuple(x) not in gone for x in q.tolist()], dtype=bool)]


def level_sets(quads, heads, L):
    """[set of the entities of level l of query b for l = 0..L] per query: the walk's node sets, from the structure alone."""
    out_of = {}
    for h, _, t, _ in np.asarray(quads, np.int64).tolist():
        out_of.setdefault(h, set()).add(t)
    levels = []
    for s in np.asarray(heads).tolist():
        cur = [{int(s)}]
        for _ in range(L):
            cur.append(set().union(*[out_of.get(x, set()) for x in cur[-1]]) if cur[-1] else set())
        levels.append(cur)
    return levels


def digraph_of(quads, heads, objs, L):
    """The r-digraphs of rows (query b, answer objs[b]) from the structure alone: (edges int64 [E, 5] = (row, hop, head, rel, tail),
    time int64 [E], reached bool [B]) ordered by (row, hop, tail, fact row): an edge of hop l is a quadruple whose head is in level
    l - 1 and whose tail leads to o in L - l steps."""
    q = np.asarray(quads, np.int64)
    levels = level_sets(q, heads, L)
    edges, times, reached = [], [], []
    for b, o in enumerate(np.asarray(objs).tolist()):
        reached.append(o in levels[b][L])
        marks, per_hop = ({o} if reached[-1] else set()), [None] * (L + 1)
        for l in range(L, 0, -1):
            ok = np.isin(q[:, 0], list(levels[b][l - 1])) & np.isin(q[:, 2], list(marks)) if marks else np.zeros(len(q), bool)
            rows = np.nonzero(ok)[0]
            per_hop[l] = rows[np.argsort(q[rows, 2], kind="stable")]
            marks = set(q[rows, 0].tolist())
        for l in range(1, L + 1):
            r = per_hop[l]
            edges.append(np.column_stack([np.full(len(r), b), np.full(len(r), l), q[r, 0], q[r, 1], q[r, 2]]).reshape(-1, 5))
            times.append(q[r, 3])
    return np.concatenate(edges, 0).astype(np.int64), np.concatenate(times).astype(np.int64), np.array(reached)


# ---- the inputs of the fidelity tests on temporal_ref.hand_graph() -------------------------------------------------------------------
# Heads: hub 2 (129 in-edges: with o = 2 a cut destination from hop 2 on), leaf 3 (the fact (3, 0, 0) at times 2 and 8 and the exact
# duplicate of the time-2 quadruple), entity 299 (identity only), 260 / 270 / 290 of 256..298, hubs 0 and 1, leaves 130, 10 and 70.
# Query times 0, 2, 8 and 11: with the edge times 0..11 past, now and future all occur on one destination (hub 2's 129 edges).
HEADS = np.array([2, 3, 299, 260, 0, 3, 130, 1, 2, 270, 3, 10, 70, 290, 2, 0])
RELS = np.array([0, 1, 6, 1, 2, 3, 5, 4, 2, 0, 6, 1, 0, 2, 5, 3])
TIMES = np.array([0, 2, 8, 11, 2, 8, 11, 0, 8, 2, 0, 11, 8, 2, 11, 0])
# the answers: o = s for the hubs and 299 (every hop then carries the hub as a destination), the fact's tail for the leaves
OBJS = np.array([2, 0, 299, 70, 0, 3, 270, 1, 2, 130, 0, 280, 260, 200, 2, 3])
# quadruples deleted, in base form (their twins go too): the duplicated (3, 0, 0, 2) - (3, 0, 0, 8) stays, so 3 still reaches 0 -, the
# only link 260 -> 70 (row 3 and row 12 are cut off), leaves of hub 2 and of hub 0, and a fact among 256..298's links
DELETED = np.array([(3, 0, 0, 2), (260, 1, 70, 4), (128, 128 % 3, 2, (128 * 5) % 12), (131, 131 % 3, 2, (131 * 5) % 12),
                    (200, 200 % 3, 2, (200 * 5) % 12), (5, 5 % 3, 0, (5 * 5) % 12), (130, 2, 270, 7)], dtype=np.int64)


def inputs(L):
    """(quads, heads, rels, times, objs, deleted) of the tests at depth L; the same rows at every depth."""
    return TR.hand_graph(), HEADS, RELS, TIMES, OBJS, DELETED
