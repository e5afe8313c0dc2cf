"""float64 per-edge walk of the temporal interpolation forward (Temporal/interpolation/model_cuda.py:137-213; shared_tables: model.py's
parameter layout) for the temporal explain / profile / predict tests: the scores and, per hop, the edge list (query, head, rel, tail,
time id) with the attention alpha of every edge - what the oracle's trace does not hold.

Every hop is written edge by edge as the reference states it: the edges are the quadruples whose head is in the query's current node
set (:141-145), dt = edge time - query time (:149), message = W_dir (h_head + rela[rel] + time_embed[|dt|]) with W_dir = future / now /
past for dt > 0 / = 0 / < 0 (:152-157), alpha = sigmoid(w2 relu(w1 [h_head | rela[rel] | rela[q_rel]])) (:159-160), new state = act(sum
of alpha * message per (query, tail)) (:175,192,196), score = linear_classifier(state) on the last node set (:210-212).
tests/test_temporal_ref.py pins the scores to the oracle's and to the reference-produced fixture."""
import numpy as np

_ACTS = {
    "tanh": np.tanh,
    "sigmoid": lambda x: 1.0 / (1.0 + np.exp(-x)),
    "relu": lambda x: np.maximum(x, 0.0),
    "idd": lambda x: x,
    "softplus": lambda x: np.logaddexp(x, 0.0),
    "leaky_relu": lambda x: np.where(x > 0, x, 0.01 * x),
}


def _np(x):
    return np.asarray(x.detach().cpu().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def direction(etime, qtime):
    """The forward's direction of an edge: 0 past (dt < 0), 1 now (dt == 0), 2 future (dt > 0), dt = edge time - query time."""
    dt = np.asarray(etime, np.int64) - np.asarray(qtime, np.int64)
    return np.where(dt > 0, 2, np.where(dt == 0, 1, 0)).astype(np.int64)


def walk(p, quads, n_ent, heads, rels, times, n_layer, act, shared_tables=False):
    """Returns (scores float64 [B, n_ent], hops, nodes): hops[l-1] = (edges int64 [E_l, 5] = (query, head, rel, tail, time id), alpha
    float64 [E_l]) of hop l, edges in (node of the current set, fact row) order; nodes = the last node set int64 [N_L, 2], sorted."""
    quads = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    heads, rels, times = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (heads, rels, times))
    B = len(heads)
    g = lambda k: _np(p[k])
    temb = g("time_embed.weight")
    W = [g("past_linear.weight"), g("now_linear.weight"), g("future_linear.weight")]       # by direction 0 / 1 / 2
    actf = _ACTS[act]
    rows_of = [[] for _ in range(n_ent)]
    for i, h in enumerate(quads[:, 0]):
        rows_of[h].append(i)
    cur = np.stack([np.arange(B), heads], 1)
    hidden = np.zeros((B, temb.shape[1]))
    hops = []
    for i in range(n_layer):
        if shared_tables:
            rela, w1, w2 = g("rela_embed.weight"), g("attention_1.weight"), g("attention_2.weight")
        else:
            rela, w1, w2 = g("rela_embed_layer.%d.weight" % i), g("attention_1_layer.%d.weight" % i), g("attention_2_layer.%d.weight" % i)
        edges, src = [], []
        for s, (b, e) in enumerate(cur):
            for row in rows_of[e]:
                edges.append((b, quads[row, 0], quads[row, 1], quads[row, 2], quads[row, 3]))
                src.append(s)
        edges, src = np.array(edges, dtype=np.int64).reshape(-1, 5), np.array(src, dtype=np.int64)
        dt = edges[:, 4] - times[edges[:, 0]]
        d_of = direction(edges[:, 4], times[edges[:, 0]])
        hs, hr = hidden[src], rela[edges[:, 2]]
        embed = hs + hr + temb[np.abs(dt)]
        msg = np.zeros_like(embed)
        for k in range(3):
            msg[d_of == k] = embed[d_of == k] @ W[k].T
        att_in = np.concatenate([hs, hr, rela[rels[edges[:, 0]]]], 1)
        alpha = 1.0 / (1.0 + np.exp(-(np.maximum(att_in @ w1.T, 0.0) @ w2.T)))          # [E, 1]
        uk, inv = np.unique(edges[:, 0] * n_ent + edges[:, 3], return_inverse=True)
        agg = np.zeros((len(uk), embed.shape[1]))
        np.add.at(agg, inv.reshape(-1), alpha * msg)
        hidden = actf(agg)
        cur = np.stack([uk // n_ent, uk % n_ent], 1)
        hops.append((edges, alpha.reshape(-1)))
    result = (hidden @ g("linear_classifier.weight").T + g("linear_classifier.bias")).reshape(-1)
    scores = np.zeros((B, n_ent))
    scores[cur[:, 0], cur[:, 1]] = result
    return scores, hops, cur


def profile_cells(hops, q_time, B, n_rows):
    """Group-by of the walk's edges: (count int64 [B, L, 3, n_rows], alpha sum float64 [B, L, 3, n_rows]) per (query, hop, direction,
    edge relation)."""
    L = len(hops)
    count = np.zeros((B, L, 3, n_rows), np.int64)
    asum = np.zeros((B, L, 3, n_rows), np.float64)
    for l, (e, al) in enumerate(hops):
        d_of = direction(e[:, 4], np.asarray(q_time, np.int64)[e[:, 0]])
        np.add.at(count, (e[:, 0], l, d_of, e[:, 2]), 1)
        np.add.at(asum, (e[:, 0], l, d_of, e[:, 2]), al)
    return count, asum


def by_relation(count, asum, rels, n_rows):
    """The per-query tables added per query relation id: [n_rows, L, 3, n_rows]."""
    c = np.zeros((n_rows,) + count.shape[1:], count.dtype)
    s = np.zeros((n_rows,) + asum.shape[1:], asum.dtype)
    np.add.at(c, np.asarray(rels, np.int64), count)
    np.add.at(s, np.asarray(rels, np.int64), asum)
    return c, s


# ---- graphs and models of the GPU tests ----------------------------------------------------------------------------------------------
class Params:
    """What T_RED_GNN's constructor reads."""

    def __init__(self, quads, n_ent, n_rela_rows, n_time, n_layer, d, a, act):
        self.graph, self.n_ent, self.n_rel, self.n_time = np.asarray(quads, np.int32), n_ent, n_rela_rows - 1, n_time
        self.n_layer, self.hidden_dim, self.attn_dim, self.act, self.device = n_layer, d, a, act, "cuda"


def make_model(quads, n_ent, n_rela_rows, n_time, n_layer, d, a, act, shared=False, seed=9, state=None):
    import torch
    from red_gnn_amd.temporal import T_RED_GNN
    torch.manual_seed(seed)
    model = T_RED_GNN(Params(quads, n_ent, n_rela_rows, n_time, n_layer, d, a, act), shared_tables=shared).cuda().eval()
    if state is not None:
        model.load_state_dict(state, strict=True)
    return model


def state_of(model):
    return {k: v.detach().cpu() for k, v in model.state_dict().items()}


HAND_N_ENT, HAND_N_REL, HAND_N_TIME = 300, 3, 12          # 300 entities: 10 bitmap words, the last one partly used


def hand_graph():
    """Quadruples with hubs 0 / 1 / 2 of in- and out-degree exactly 64 / 65 / 129 (identity edge included; the neighbours are leaves of
    their own, 3..63, 64..127 and 128..255, linked in both directions), entity 299 of degree 1 (identity only), the fact (3, 0, 0) at
    times 2 and 8 with the time-2 quadruple given twice (an exact duplicate; all three count towards hub 0's 64), random facts among
    256..298 and four links between leaves and those.  Relations 0..2, inverses 3..5, identity 6 at time n_time - 1.
    Returns int64 [n, 4]."""
    rng = np.random.default_rng(5)
    R, T = HAND_N_REL, HAND_N_TIME
    rows = []
    for hub, lo, hi in ((0, 3, 64), (1, 64, 128), (2, 128, 256)):
        rows += [(leaf, leaf % R if leaf != 3 else 0, hub, (leaf * 5) % T if leaf != 3 else 2) for leaf in range(lo, hi)]
    rows += [(3, 0, 0, 8), (3, 0, 0, 2)]
    h, t = rng.integers(256, 299, 120), rng.integers(256, 299, 120)
    rows += list(zip(h.tolist(), rng.integers(0, R, 120).tolist(), t.tolist(), rng.integers(0, T, 120).tolist()))
    rows += [(260, 1, 70, 4), (130, 2, 270, 7), (10, 0, 280, 0), (290, 2, 200, 11)]
    q = np.array(rows, dtype=np.int64)
    ent = np.arange(HAND_N_ENT)
    quads = np.concatenate([q, np.column_stack([q[:, 2], q[:, 1] + R, q[:, 0], q[:, 3]]),
                            np.column_stack([ent, np.full(len(ent), 2 * R), ent, np.full(len(ent), T - 1)])], 0)
    indeg, outdeg = np.bincount(quads[:, 2], minlength=HAND_N_ENT), np.bincount(quads[:, 0], minlength=HAND_N_ENT)
    assert indeg[[0, 1, 2, 299]].tolist() == [64, 65, 129, 1] and outdeg[[0, 1, 2, 299]].tolist() == [64, 65, 129, 1]
    return quads


def csr_positions(graph, rec):
    """CSR-by-tail position of every record (head, rel, tail, time) of int64 [n, 4], from the device graph's export() and
    export_time(); the k-th occurrence of a record that the graph holds several times (an exact duplicate quadruple) takes the k-th of
    its positions, in the order given."""
    _, _, ip, ihr = graph.export()
    _, it = graph.export_time()
    where = {}
    for t in np.unique(rec[:, 2]).tolist():
        for q in range(ip[t], ip[t + 1]):
            where.setdefault((int(ihr[q, 0]), int(ihr[q, 1]), t, int(it[q])), []).append(q)
    return where


def expected_digraph(hops, q_of, objs, last_nodes, tau, n_ent, graph):
    """r-digraphs of rows (query q_of[i], answer objs[i]) from the walk's hops: (edges int64 [E, 5] = (row, hop, head, rel, tail),
    time [E], alpha [E], offsets [B + 1], reached [B]) ordered by (row, hop, tail, CSR-by-tail position)."""
    from tests import explain_ref as X
    L, B = len(hops), len(q_of)
    last = set(map(tuple, np.asarray(last_nodes).tolist()))
    reached = np.array([(int(q_of[i]), int(objs[i])) in last for i in range(B)])
    parts, alphas = [], []
    for l, (e, al) in enumerate(hops):
        for i, q in enumerate(q_of):
            m = e[:, 0] == q
            parts.append(np.column_stack([np.full(m.sum(), i), np.full(m.sum(), l + 1), e[m, 1:5]]))
            alphas.append(al[m])
    cat, al = np.concatenate(parts, 0), np.concatenate(alphas)
    row, hop, head, rel, tail, tm = cat.T
    ok = X.rdigraph_mask(row, hop, head, tail, al, objs, reached, tau, n_ent, L)
    cat, al = cat[ok], al[ok]
    where = csr_positions(graph, cat[:, 2:6]) if len(cat) else {}
    taken, pos = {}, np.zeros(len(cat), np.int64)
    for i, (r, hp, h, rl, t, m) in enumerate(cat.tolist()):
        k = taken.get((r, hp, h, rl, t, m), 0)
        taken[(r, hp, h, rl, t, m)] = k + 1
        pos[i] = where[(h, rl, t, m)][k]
    o = np.lexsort((pos, cat[:, 4], cat[:, 1], cat[:, 0]))
    cat, al = cat[o], al[o]
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(cat[:, 0], minlength=B)) if len(cat) else 0
    return cat[:, :5], cat[:, 5], al, offsets, reached
