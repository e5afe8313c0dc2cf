"""Plain-numpy reference of RDigraph.rescore, fact_mask and data_row_mask on an extrapolation r-digraph, and the inputs the
extrapolation fidelity tests share.  TEST INFRASTRUCTURE.

rescore: the arithmetic of tests/extrap_ref.walk (un-hoisted: W_past applied per edge to h_head + rela[rel] + periodic_embedding(lag),
the same attention) over an explicit edge list (row, hop, head, rel, tail) with a day per edge, under a keep mask and with the forward
liveness sweep of tests/rescore_ref.py: a kept hop-l edge carries a message iff its head is a node of hop l - 1, hop 0 being (row, s).
``dtype`` np.float64 is the reference, np.float32 the yardstick of what an fp32 evaluation costs.  Nothing here is taken from the
library: a row's digraph is cut out of the walk's own per-hop edge lists (digraph_of).
"""
import numpy as np

from tests import extrap_ref as XR
from tests.temporal_ref import _ACTS
from tests.trescore_ref import _find, _sigmoid

GRANULARITY = 24
CHUNK = 128                                              # RG_DIGRAPH_CHUNK: a destination of more edges is cut


def rescore(p, edges, day, q_day, heads, rels, n_ent, n_layer, act, keep=None, dtype=np.float64):
    """(score [B], reached bool [B], live bool [E], alpha [E]) of the rows' answers on the kept edges.  ``edges`` int [E, 5] = (row,
    hop, head, rel, tail) with ``day`` int [E] the day the forward used for the edge and ``q_day`` int [B] the rows' query days; the
    hop-L edges of a row share their tail, the row's answer.  ``p``: a state dict of extrapolation.T_RED_GNN (arrays or tensors)."""
    dt_ = np.dtype(dtype)
    g = lambda k: np.asarray(p[k].detach().cpu().numpy() if hasattr(p[k], "detach") else p[k]).astype(dt_)
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    row, hop, head, rel, tail = e.T
    day, q_day = np.asarray(day, np.int64), np.asarray(q_day, np.int64).reshape(-1)
    heads, rels = (np.asarray(x, np.int64).reshape(-1) for x in (heads, rels))
    w_past = g("past_linear.weight")
    pt = {k: g(k) for k in p if k.startswith("time_embed.")}
    B, E, d = len(heads), len(e), w_past.shape[0]
    keep = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    score, reached = np.zeros(B, dt_), np.zeros(B, bool)
    live, alpha = np.zeros(E, bool), np.zeros(E, dt_)
    keys_prev = np.arange(B) * n_ent + heads
    hidden = np.zeros((B, d), dt_)
    for l in range(1, n_layer + 1):
        rela, w1, w2 = (g("%s.%d.weight" % (name, l - 1)) for name in ("rela_embed_layer", "attention_1_layer", "attention_2_layer"))
        at = np.nonzero((hop == l) & keep)[0]
        src, ok = _find(keys_prev, row[at] * n_ent + head[at])
        at, src = at[ok], src[ok]
        if len(at) == 0:
            return score, reached, live, alpha
        live[at] = True
        keys, dst = np.unique(row[at] * n_ent + tail[at], return_inverse=True)
        hs, hr = hidden[src], rela[rel[at]]
        temb = XR.periodic_embedding(pt, "time_embed.", (q_day[row[at]] - day[at]).astype(dt_)).astype(dt_)
        msg = (hs + hr + temb) @ w_past.T
        att_in = np.concatenate([hs, hr, rela[rels[row[at]]]], 1)
        al = _sigmoid(np.maximum(att_in @ w1.T, 0) @ w2.T).astype(dt_)
        alpha[at] = al[:, 0]
        agg = np.zeros((len(keys), d), dt_)
        np.add.at(agg, dst.reshape(-1), al * msg)
        hidden = _ACTS[act](agg).astype(dt_)
        keys_prev = keys
    rows = keys_prev // n_ent
    assert len(np.unique(rows)) == len(rows), "the hop-L edges of a row must share their tail"
    score[rows] = (hidden @ g("linear_classifier.weight").T + g("linear_classifier.bias"))[:, 0]
    reached[rows] = True
    return score, reached, live, alpha


def twin(s, p, o, day, m):
    return (o, p + m if p < m else p - m, s, day)


def fact_mask(edges, day, data_row, n_rel, facts, rows=None, inverse_offset=None):
    """bool [E]: the data-row edge (row, hop, head, rel, tail) of day ``day`` is a fact (s, p, o, day) of its row (``rows[f]``; None:
    of any row) or, with ``inverse_offset`` = m, its twin; a self-loop (data row -1, relation ``n_rel``) is never marked."""
    want = set()
    for f, (s, p, o, dy) in enumerate(np.asarray(facts, np.int64).reshape(-1, 4).tolist()):
        if p == n_rel:
            continue
        b = -1 if rows is None else int(rows[f])
        want.add((b, s, p, o, dy))
        if inverse_offset is not None:
            want.add((b,) + twin(s, p, o, dy, inverse_offset))
    e = np.asarray(edges, np.int64).reshape(-1, 5).tolist()
    return np.array([r >= 0 and rel != n_rel and ((-1 if rows is None else b), h, rel, t, int(dy)) in want
                     for (b, _, h, rel, t), dy, r in zip(e, np.asarray(day).tolist(), np.asarray(data_row).tolist())], dtype=bool)


def data_row_mask(edges, data_row, data_rows, rows=None):
    """bool [E]: the edge's data row is listed (for its row, with ``rows``)."""
    want = {(-1 if rows is None else int(rows[f]), int(r)) for f, r in enumerate(np.asarray(data_rows).tolist())}
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    return np.array([r >= 0 and ((-1 if rows is None else int(b)), int(r)) in want for b, r in zip(e[:, 0].tolist(), np.asarray(data_row).tolist())],
                    dtype=bool)


def rows_of_facts(data, facts, granularity=GRANULARITY):
    """The data rows that ARE one of the facts (s, p, o, day): every copy, at any hour of the day."""
    data = np.asarray(data, np.int64)
    want = set(map(tuple, np.asarray(facts, np.int64).reshape(-1, 4).tolist()))
    return np.array([i for i, (s, p, o, ts) in enumerate(data.tolist()) if (s, p, o, ts // granularity) in want], dtype=np.int64)


def without_rows(data, rows):
    """``data`` without the rows ``rows``."""
    keep = np.ones(len(data), bool)
    keep[np.asarray(rows, np.int64)] = False
    return np.asarray(data)[keep]


def digraph_of(hops, q_of, objs, last_nodes, n_ent):
    """The r-digraphs of rows (query q_of[i], answer objs[i]) from extrap_ref.walk's hops: (edges int64 [E, 5] = (row, hop, head, rel,
    tail), data_row [E], day [E], reached [B]) ordered by (row, hop, tail, data row; the self-loop, -1, first): an edge of hop l is a
    walked edge whose tail leads to o in L - l steps."""
    L = len(hops)
    last = set(map(tuple, np.asarray(last_nodes).tolist()))
    parts, reached = [], []
    for i, (q, o) in enumerate(zip(np.asarray(q_of).tolist(), np.asarray(objs).tolist())):
        reached.append((q, o) in last)
        marks = {o} if reached[-1] else set()
        per_hop = [None] * L
        for l in range(L, 0, -1):
            e, _, dy = hops[l - 1]
            m = (e[:, 0] == q) & np.isin(e[:, 3], list(marks)) if marks else np.zeros(len(e), bool)
            per_hop[l - 1] = np.column_stack([np.full(m.sum(), i), np.full(m.sum(), l), e[m, 1], e[m, 2], e[m, 3], e[m, 4], dy[m]]).reshape(-1, 7)
            marks = set(e[m, 1].tolist())
        for x in per_hop:
            parts.append(x[np.lexsort((x[:, 5], x[:, 4]))])
    cat = np.concatenate(parts, 0).astype(np.int64)
    return cat[:, :5], cat[:, 5], cat[:, 6], np.array(reached)


# ---- the inputs of the fidelity tests on extrap_ref.make_case ---------------------------------------------------------------------------
def rows_of_case(q, hops, last_nodes, data, rng_seed=0):
    """(q_of, objs), the rows (query, answer) over queries_of_case's queries: test_temporal_explain_gpu._rows on the walk's last
    level for the case's own queries, the duplicated rows' object for the query over them, and entity 0 - the hub object: about a
    sixth of all rows end there - for the three queries with the most hop-L edges into it.  ``hops``: extrap_ref.walk's."""
    from tests.test_temporal_explain_gpu import _rows
    B = len(q) - 2
    q_of, objs = _rows(last_nodes[last_nodes[:, 0] < B], B, XR.N_ENT, np.random.default_rng(rng_seed), per_query=2 if B > 9 else 3)
    rows = set(zip(q_of.tolist(), objs.tolist())) | {(B, int(data[9, 2]))}
    e = hops[-1][0]
    into_hub = np.bincount(e[e[:, 3] == 0, 0], minlength=len(q))
    rows |= {(int(b), 0) for b in np.argsort(-into_hub, kind="stable")[:3] if into_hub[b]}
    rows = np.array(sorted(rows), dtype=np.int64)
    return rows[:, 0], rows[:, 1]


def queries_of_case(data, q):
    """The case's queries, one over the duplicated rows 9..13 (their (s, p) five days later) and one of the busiest subject on the
    day after the last row, whose window is full."""
    data = np.asarray(data, np.int64)
    s, p, o, t = data[9]
    busiest = int(np.bincount(data[:, 0]).argmax())
    return np.concatenate([q, [[s, p, o, t + 5 * GRANULARITY], [busiest, 0, 0, (data[-1, 3] // GRANULARITY) * GRANULARITY]]], 0)


def deleted_facts(data, edges, data_row, day, heads, granularity=GRANULARITY):
    """The facts (s, p, o, day) the tests delete, chosen from the digraph by a rule that reads no score: data row 9 (one of the five
    equal rows), and for every fourth row of the digraph (rows 1, 5, 9, ..) whose answer is not its subject every fact that leaves
    the subject at hop 1 - the row is then cut off and its later hops dangle - except the facts one of whose data rows is the last
    row of its day (deleting it would move a window boundary, see RDigraph.rescore)."""
    data = np.asarray(data, np.int64)
    day_of = data[:, 3] // granularity
    last_of_day = set(np.nonzero(np.append(day_of[1:] != day_of[:-1], True))[0].tolist())
    facts = {tuple(data[9, :3].tolist()) + (int(day_of[9]),)}
    B = len(heads)
    for b in range(1, B, 4):
        m = (edges[:, 0] == b) & (edges[:, 1] == 1) & (data_row >= 0)
        answer = edges[(edges[:, 0] == b)][-1, 4] if (edges[:, 0] == b).any() else heads[b]
        if answer == heads[b]:
            continue
        for (h, r, t), dy in zip(edges[m][:, 2:5].tolist(), day[m].tolist()):
            facts.add((h, r, t, int(dy)))
    out = []
    for f in sorted(facts):
        if not set(rows_of_facts(data, [f], granularity).tolist()) & last_of_day:
            out.append(f)
    return np.array(out, np.int64).reshape(-1, 4)
