"""References of the extrapolation model's predict / explain tests (extrapolation.py) in numpy.

``walk`` is a float64 per-edge walk of the forward (Temporal/extrapolation/model_cuda_new_embedding.py:135-261): per query the window
dataset[time_offset_list[begin]:time_offset_list[cur_t]] with begin = max(cur_t - 120, 0) and a self-loop (e, n_rel, e) at day `begin`
for every entity (:165-176); per hop the window's rows whose subject is in the query's node set (:186-189), message = W_past (h_s +
rela[rel] + time_embed(cur_t - day)) (:192-205), alpha = sigmoid(w2 relu(w1 [h_s | rela[rel] | rela[q_rel]])) (:207-208), new state =
act(sum of alpha * message per (query, object)) (:224-238), logits = linear_classifier(state) (:244).  It returns what the oracle's
restatement does not hold: every hop's edges with their data row and alpha.  tests/test_extrap_ref.py pins its logits and node sets to
the oracle's extrap_forward in float64.

``segment_topk_ref`` restates rg_segment_topk's contract: per query the pairs of its segment whose entity is not in the key's
known-object list, ordered by score descending (NaN lowest, -0 == +0) and entity id ascending, with the float64 softmax over the whole
segment (scatter_softmax, :248)."""
import numpy as np

from tests.temporal_ref import _ACTS, _np

WINDOW = 120


def periodic_embedding(p, prefix, x):
    """The reference's edited PeriodicEmbeddings (rtdl_num_embeddings.py:92-100,199-215), one feature: x [N] -> [N, d]."""
    g = lambda k: _np(p[prefix + k])
    x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
    z = 2 * np.pi * g("periodic.weight") * x                                   # [N, k]
    z = np.concatenate([np.cos(z), np.sin(z)], 1)
    neg = z @ g("linear_neg.weight")[0] + g("linear_neg.bias")
    pos = z @ g("linear_pos.weight")[0] + g("linear_pos.bias")
    return np.maximum(np.where(x < 0, neg, pos), 0.0)


def walk(p, data, time_offset_list, time_granularity, n_ent, n_rel_true, src, rel, ts, n_layer, act):
    """Returns (logits float64 [N], nodes int64 [N, 2] = the last node set, sorted, hops, cur_t): hops[l-1] = (edges int64 [E_l, 5] =
    (query, head, rel, tail, data row; -1 for a self-loop), alpha float64 [E_l], day int64 [E_l] = the edge's day: the row's, or the
    window's first day for a self-loop) of hop l."""
    data = np.asarray(data, dtype=np.int64).reshape(-1, 4)
    src, rel, ts = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (src, rel, ts))
    off = np.asarray(time_offset_list, dtype=np.int64)
    B = len(src)
    g = lambda k: _np(p[k])
    w_past = g("past_linear.weight")
    cur_t = ts // time_granularity
    begin = np.maximum(cur_t - WINDOW, 0)
    day_of = data[:, 3] // time_granularity
    rows_of = []                                   # per query: subject -> data rows of its window, in row order
    for b in range(B):
        by = {}
        for row in range(off[begin[b]], off[cur_t[b]]):
            by.setdefault(int(data[row, 0]), []).append(row)
        rows_of.append(by)
    cur = np.stack([np.arange(B), src], 1)
    hidden = np.zeros((B, w_past.shape[0]))
    hops = []
    for i in range(n_layer):
        rela, w1, w2 = g("rela_embed_layer.%d.weight" % i), g("attention_1_layer.%d.weight" % i), g("attention_2_layer.%d.weight" % i)
        edges, day, pos = [], [], []
        for s, (b, e) in enumerate(cur.tolist()):
            edges.append((b, e, n_rel_true, e, -1)); day.append(begin[b]); pos.append(s)
            for row in rows_of[b].get(e, ()):
                edges.append((b, e, data[row, 1], data[row, 2], row)); day.append(day_of[row]); pos.append(s)
        edges, day, pos = np.array(edges, dtype=np.int64).reshape(-1, 5), np.array(day, dtype=np.int64), np.array(pos, dtype=np.int64)
        hs, hr = hidden[pos], rela[edges[:, 2]]
        msg = (hs + hr + periodic_embedding(p, "time_embed.", cur_t[edges[:, 0]] - day)) @ w_past.T
        att_in = np.concatenate([hs, hr, rela[rel[edges[:, 0]]]], 1)
        alpha = 1.0 / (1.0 + np.exp(-(np.maximum(att_in @ w1.T, 0.0) @ w2.T)))               # [E, 1]
        uk, inv = np.unique(edges[:, 0] * n_ent + edges[:, 3], return_inverse=True)
        agg = np.zeros((len(uk), msg.shape[1]))
        np.add.at(agg, inv.reshape(-1), alpha * msg)
        hidden = _ACTS[act](agg)
        cur = np.stack([uk // n_ent, uk % n_ent], 1)
        hops.append((edges, alpha.reshape(-1), day))
    logits = (hidden @ g("linear_classifier.weight").T + g("linear_classifier.bias")).reshape(-1)
    return logits, cur, hops, cur_t


def expected_digraph(hops, q_of, objs, last_nodes, tau, n_ent, n_data, graph):
    """r-digraphs of rows (query q_of[i], answer objs[i]) from the walk's hops: (edges int64 [E, 5] = (row, hop, head, rel, tail),
    data_row [E], day [E], alpha [E], offsets [B + 1], reached [B]) ordered by (row, hop, tail, CSR-by-tail position); the CSR order
    comes from the device graph's export (its time field is the data row, n_data for the self-loops)."""
    from tests import explain_ref as X
    L, B = len(hops), len(q_of)
    last = set(map(tuple, np.asarray(last_nodes).tolist()))
    reached = np.array([(int(q_of[i]), int(objs[i])) in last for i in range(B)])
    parts, alphas, days = [], [], []
    for l, (e, al, dy) in enumerate(hops):
        for i, q in enumerate(q_of):
            m = e[:, 0] == q
            parts.append(np.column_stack([np.full(m.sum(), i), np.full(m.sum(), l + 1), e[m, 1:5]]))
            alphas.append(al[m]); days.append(dy[m])
    cat, al, dy = np.concatenate(parts, 0), np.concatenate(alphas), np.concatenate(days)
    ok = X.rdigraph_mask(cat[:, 0], cat[:, 1], cat[:, 2], cat[:, 4], al, objs, reached, tau, n_ent, L)
    cat, al, dy = cat[ok], al[ok], dy[ok]
    _, _, ip, ihr = graph.export()
    _, it = graph.export_time()
    where = {}
    for t in np.unique(cat[:, 4]).tolist():
        for c in range(ip[t], ip[t + 1]):
            where[(int(ihr[c, 0]), int(ihr[c, 1]), t, int(it[c]))] = c          # (the row id makes every entry unique)
    pos = np.array([where[(h, r, t, n_data if row < 0 else row)] for h, r, t, row in cat[:, 2:6].tolist()], dtype=np.int64)
    o = np.lexsort((pos, cat[:, 4], cat[:, 1], cat[:, 0]))
    cat, al, dy = cat[o], al[o], dy[o]
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(cat[:, 0], minlength=B)) if len(cat) else 0
    return cat[:, :5], cat[:, 5], dy, al, offsets, reached


# ---- the graph and the models of the GPU tests ------------------------------------------------------------------------------------------
N_ENT, N_REL, N_ROWS = 150, 6, 6000
CASES = [(32, 5, "tanh", 3, 9), (64, 30, "relu", 2, 24), (20, 3, "idd", 2, 3)]      # (d, a, act, L, B)


def make_case(d, B):
    """The graph of test_gpu_parity.test_temporal_extrapolation_training_step_vs_oracle_autograd: 150 entities, 6 relations, 6000 rows
    over 220 days with days without rows, hub subjects and objects, rows 9..13 equal, and B queries older and younger than the
    window.  Returns (data int64 [n, 4], queries int64 [B, 4])."""
    rng = np.random.default_rng(7 * d + B)
    days = np.sort(rng.choice(np.delete(np.arange(220), [0, 50, 51, 120]), N_ROWS))
    w = 1.0 / np.arange(1, N_ENT + 1); w /= w.sum()
    data = np.stack([rng.choice(N_ENT, N_ROWS, p=w[::-1]), rng.integers(0, N_REL, N_ROWS), rng.choice(N_ENT, N_ROWS, p=w),
                     days * 24 + rng.integers(0, 24, N_ROWS)], 1)
    data = data[np.argsort(data[:, 3], kind="stable")]
    data[10:14] = data[9]
    q = data[np.sort(rng.choice(np.arange(30, N_ROWS), B, replace=False))]
    return data, q


class Params:
    """What extrapolation.T_RED_GNN's constructor reads."""

    def __init__(self, data, d, a, act, n_layer, device="cuda"):
        self.n_ent, self.n_rel, self.data, self.time_granularity = N_ENT, N_REL, data, 24
        self.hidden_dim, self.attn_dim, self.n_layer, self.act, self.device = d, a, n_layer, act, device


def make_model(data, d, a, act, n_layer, seed=3):
    import torch
    from red_gnn_amd import extrapolation as X
    torch.manual_seed(seed)
    return X.T_RED_GNN(Params(data, d, a, act, n_layer)).cuda().eval()


class Batch:
    def __init__(self, q):
        q = np.asarray(q)
        self.src_idx, self.rel_idx, self.ts = q[:, 0], q[:, 1], q[:, 3]


def key32(x):
    """Order-preserving uint32 key of float32 scores: NaN lowest, -0 == +0 (csrc/select.h)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    k = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(x)] = 0
    return k


def known_list(known, key):
    """The objects of ``key`` in a (keys, ptr, idx) index; empty when the index is None or lacks the key."""
    if known is None or len(known[0]) == 0:
        return np.zeros(0, np.int64)
    keys, ptr, idx = (np.asarray(a) for a in known)
    i = int(np.searchsorted(keys, key))
    if i == len(keys) or keys[i] != key:
        return np.zeros(0, np.int64)
    return idx[ptr[i]:ptr[i + 1]].astype(np.int64)


def segment_topk_ref(scores, ent, seg_ptr, k, q_key=None, known=None):
    """(ids int32 [B, k], scores float32 [B, k], prob float64 [B, k]) with -1 / -inf / 0 past a query's kept pairs."""
    scores, ent = np.asarray(scores, dtype=np.float32), np.asarray(ent, dtype=np.int64)
    seg_ptr = np.clip(np.asarray(seg_ptr, dtype=np.int64), 0, len(scores))
    B = len(seg_ptr) - 1
    ids = np.full((B, k), -1, np.int32)
    val = np.full((B, k), -np.inf, np.float32)
    prob = np.zeros((B, k), np.float64)
    for q in range(B):
        lo, hi = seg_ptr[q], max(seg_ptr[q + 1], seg_ptr[q])
        s, e = scores[lo:hi], ent[lo:hi]
        if len(s) == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            s64 = s.astype(np.float64)
            p = np.exp(s64 - np.max(s64))            # (np.max propagates a NaN)
            p = p / p.sum()
        keep = ~np.isin(e, known_list(known, None if q_key is None else q_key[q]))
        order = np.lexsort((e, -key32(s).astype(np.int64)))
        order = order[keep[order]][:k]
        n = len(order)
        ids[q, :n], val[q, :n], prob[q, :n] = e[order], s[order], p[order]
    return ids, val, prob
