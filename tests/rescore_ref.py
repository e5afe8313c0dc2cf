"""Plain-numpy reference of RDigraph.rescore and RDigraph.fact_mask, and the cases the fidelity tests share.  TEST INFRASTRUCTURE.

rescore: RED-GNN's forward (oracle.redgnn_oracle.forward's arithmetic, un-hoisted: the three attention Linear layers applied per edge)
over an explicit edge list (row, hop, head, rel, tail) under a keep mask, with the forward liveness sweep: a kept hop-l edge carries a
message iff its head is a node of hop l - 1, hop 0 being (row, s).  ``dtype`` np.float64 is the reference, np.float32 the yardstick of
what an fp32 evaluation costs.  Nothing here is taken from the library: the digraph of a row is cut out of the oracle's own per-hop
edge lists (digraph_of), ordered by (row, hop, tail, fact row).
"""
import types

import numpy as np
import torch

from oracle import redgnn_oracle as orc

_ACTS = {"relu": lambda x: np.maximum(x, 0), "tanh": np.tanh, "idd": lambda x: x}


def random_params(seed, n_layer, d, attn, n_rel):
    """A state dict of RED_GNN_trans's names and shapes (float32 numpy), N(0, 0.3)."""
    rng = np.random.default_rng(seed)
    f = lambda *shape: (rng.standard_normal(shape) * 0.3).astype(np.float32)
    p = {"W_final.weight": f(1, d), "gate.weight_ih_l0": f(3 * d, d), "gate.weight_hh_l0": f(3 * d, d), "gate.bias_ih_l0": f(3 * d),
         "gate.bias_hh_l0": f(3 * d)}
    for i in range(n_layer):
        pre = "gnn_layers.%d." % i
        p.update({pre + "rela_embed.weight": f(2 * n_rel + 1, d), pre + "Ws_attn.weight": f(attn, d), pre + "Wr_attn.weight": f(attn, d),
                  pre + "Wqr_attn.weight": f(attn, d), pre + "Wqr_attn.bias": f(attn), pre + "w_alpha.weight": f(1, attn),
                  pre + "w_alpha.bias": f(1), pre + "W_h.weight": f(d, d)})
    return p


def _find(keys, want):
    if len(keys) == 0:
        return np.zeros(len(want), np.int64), np.zeros(len(want), bool)
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return pos, keys[pos] == want


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def rescore(p, edges, q_sub, q_rel, n_ent, L, act, keep=None, dtype=np.float64):
    """(score [B], reached bool [B], live bool [E], alpha [E]) of the rows' answers on the kept edges.  ``edges`` int [E, 5] = (row,
    hop, head, rel, tail) ordered by (row, hop, tail, ...); the hop-L edges of a row share their tail, the row's answer."""
    dt = np.dtype(dtype)
    g = lambda k: np.asarray(p[k]).astype(dt)
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    row, hop, head, rel, tail = e.T
    q_sub, q_rel = np.asarray(q_sub, np.int64), np.asarray(q_rel, np.int64)
    B, E, d = len(q_sub), len(e), g("W_final.weight").shape[1]
    keep = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    score, reached = np.zeros(B, dt), np.zeros(B, bool)
    live, alpha = np.zeros(E, bool), np.zeros(E, dt)
    keys_prev = np.arange(B) * n_ent + q_sub
    hidden = np.zeros((B, d), dt)
    w_ih, w_hh, b_ih, b_hh = g("gate.weight_ih_l0"), g("gate.weight_hh_l0"), g("gate.bias_ih_l0"), g("gate.bias_hh_l0")
    for l in range(1, L + 1):
        pre = "gnn_layers.%d." % (l - 1)
        at = np.nonzero((hop == l) & keep)[0]
        src, ok = _find(keys_prev, row[at] * n_ent + head[at])
        at, src = at[ok], src[ok]
        if len(at) == 0:
            return score, reached, live, alpha
        live[at] = True
        keys, dst = np.unique(row[at] * n_ent + tail[at], return_inverse=True)
        rela = g(pre + "rela_embed.weight")
        hs, hr, hq = hidden[src], rela[rel[at]], rela[q_rel[row[at]]]
        z = hs @ g(pre + "Ws_attn.weight").T + hr @ g(pre + "Wr_attn.weight").T + hq @ g(pre + "Wqr_attn.weight").T + g(pre + "Wqr_attn.bias")
        al = _sigmoid(np.maximum(z, 0) @ g(pre + "w_alpha.weight").T + g(pre + "w_alpha.bias")).astype(dt)
        alpha[at] = al[:, 0]
        agg = np.zeros((len(keys), d), dt)
        np.add.at(agg, dst, al * (hs + hr))
        x = _ACTS[act](agg @ g(pre + "W_h.weight").T)
        pos, had = _find(keys_prev, keys)
        h0 = np.zeros((len(keys), d), dt)
        h0[had] = hidden[pos[had]]
        gi, gh = x @ w_ih.T + b_ih, h0 @ w_hh.T + b_hh
        r_, z_ = _sigmoid(gi[:, :d] + gh[:, :d]), _sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
        n_ = np.tanh(gi[:, 2 * d:] + r_ * gh[:, 2 * d:])
        hidden = ((1 - z_) * n_ + z_ * h0).astype(dt)
        keys_prev = keys
    rows = keys_prev // n_ent
    assert len(np.unique(rows)) == len(rows), "the hop-L edges of a row must share their tail"
    score[rows] = (hidden @ g("W_final.weight").T)[:, 0]
    reached[rows] = True
    return score, reached, live, alpha


def inverse(r, n_rel):
    return r + n_rel if r < n_rel else r - n_rel


def fact_mask(edges, n_rel, facts, rows=None):
    """bool [E]: edge (row, hop, head, rel, tail) is a fact (h, r, t) of its row (``rows[f]``; None: of any row) or its twin (t, inv(r),
    h); the identity relation 2 * n_rel is never marked."""
    want = set()
    for f, (h, r, t) in enumerate(np.asarray(facts, np.int64).reshape(-1, 3).tolist()):
        if r == 2 * n_rel:
            continue
        b = -1 if rows is None else int(rows[f])
        want.add((b, h, r, t))
        want.add((b, t, inverse(r, n_rel), h))
    return np.array([rel != 2 * n_rel and ((-1 if rows is None else b), h, rel, t) in want
                     for b, _, h, rel, t in np.asarray(edges, np.int64).reshape(-1, 5).tolist()], dtype=bool)


def digraph_of(trace, q_of, objs, n_ent):
    """The r-digraphs of rows (query q_of[i], answer objs[i]) cut from the oracle's per-hop edges ``trace`` (forward(trace=...)):
    (edges int64 [E, 5] ordered by (row, hop, tail, fact-row order), offsets [B + 1], reached bool [B]).  Backward marks from o, as
    tests/explain_ref.rdigraph_mask states the definition."""
    L, B = len(trace), len(q_of)
    last = trace[-1]["nodes"]
    member = set(map(tuple, last.tolist()))
    reached = np.array([(int(q_of[i]), int(objs[i])) in member for i in range(B)])
    out = []
    for i in range(B):
        per_hop = [None] * (L + 1)
        marks = {int(objs[i])} if reached[i] else set()
        for l in range(L, 0, -1):
            e = trace[l - 1]["edges"]
            e = e[e[:, 0] == q_of[i]]
            e = e[np.isin(e[:, 3], list(marks))] if marks else e[:0]
            per_hop[l] = e[np.argsort(e[:, 3], kind="stable")]
            marks = set(e[:, 1].tolist())
        for l in range(1, L + 1):
            e = per_hop[l]
            out.append(np.stack([np.full(len(e), i), np.full(len(e), l), e[:, 1], e[:, 2], e[:, 3]], 1).reshape(-1, 5))
    edges = np.concatenate(out, 0).astype(np.int64) if out else np.zeros((0, 5), np.int64)
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(edges[:, 0], minlength=B))
    return edges, offsets, reached


def base_fact(head, rel, tail, n_rel):
    """The triple (h, r, t) with r < n_rel behind a non-identity edge."""
    return (head, rel, tail) if rel < n_rel else (tail, rel - n_rel, head)


def without_facts(triples, facts):
    """``triples`` int [T, 3] (base relations) without every copy of the base triples ``facts``."""
    gone = set(map(tuple, np.asarray(facts, np.int64).reshape(-1, 3).tolist()))
    t = np.asarray(triples, np.int64)
    return t[np.array([tuple(x) not in gone for x in t.tolist()], dtype=bool)] if len(t) else t


def make_case(name, n_ent, n_rel, n_tri, L, d, attn, act, B, n_del, seed):
    """A knowledge graph of ``n_tri`` random triples, ``B`` rows (s, r, o) with o in the level-L set of (s, r), their digraphs, and per
    row ``n_del`` facts of its digraph picked for deletion (all of them where it has fewer).  Everything from the oracle."""
    rng = np.random.default_rng(seed)
    tri = np.stack([rng.integers(0, n_ent, n_tri), rng.integers(0, n_rel, n_tri), rng.integers(0, n_ent, n_tri)], 1)
    tri = np.concatenate([tri, tri[:5]], 0)                                # a few parallel facts
    p = random_params(seed + 1, L, d, attn, n_rel)
    og = orc.OracleGraph(orc.double_triple(tri, n_rel), n_ent, n_rel)
    subs, rels = rng.integers(0, n_ent, B), rng.integers(0, 2 * n_rel, B)
    trace = []
    pt = {k: torch.as_tensor(v) for k, v in p.items()}
    scores = orc.forward(pt, og, subs, rels, L, act=act, dtype=torch.float64, trace=trace).numpy()
    last = trace[-1]["nodes"]
    objs = np.array([rng.choice(last[last[:, 0] == b, 1]) for b in range(B)])
    edges, offsets, reached = digraph_of(trace, np.arange(B), objs, n_ent)
    assert reached.all()
    facts, rows = [], []
    for b in range(B):
        mine = edges[offsets[b]:offsets[b + 1]]
        distinct = sorted({base_fact(h, r, t, n_rel) for _, _, h, r, t in mine.tolist() if r != 2 * n_rel})
        for j in rng.permutation(len(distinct))[:n_del]:
            facts.append(distinct[j])
            rows.append(b)
    return types.SimpleNamespace(name=name, n_ent=n_ent, n_rel=n_rel, triples=tri, L=L, d=d, attn=attn, act=act, B=B, params=p, og=og,
                                 subs=subs, rels=rels, objs=objs, edges=edges, offsets=offsets, scores=scores,
                                 facts=np.array(facts, np.int64).reshape(-1, 3), fact_rows=np.array(rows, np.int64))


def oracle_without(case, b, dtype=torch.float64):
    """(score of o, o in the last level, [set of the entities of level l for l = 0..L]) of row b from oracle.forward on the graph rebuilt
    without the row's deleted facts."""
    gone = case.facts[case.fact_rows == b]
    og = orc.OracleGraph(orc.double_triple(without_facts(case.triples, gone), case.n_rel), case.n_ent, case.n_rel)
    trace = []
    pt = {k: torch.as_tensor(v) for k, v in case.params.items()}
    s = orc.forward(pt, og, case.subs[b:b + 1], case.rels[b:b + 1], case.L, act=case.act, dtype=dtype, trace=trace).numpy()
    levels = [{int(case.subs[b])}] + [set(t["nodes"][:, 1].tolist()) for t in trace]
    return s[0, case.objs[b]], int(case.objs[b]) in levels[-1], levels


# name -> arguments of make_case.  The 300-entity graphs are the shape of the GPU tests' synthetic KG; on the 60-entity graph most
# deletions disconnect.  Seeds and deletion counts are chosen so that in every case at least a quarter of the rows stay reached and at
# least one becomes unreached (test_rescore_ref.py asserts both with this reference alone).
CASES = {
    "e300_L2": dict(n_ent=300, n_rel=7, n_tri=3000, L=2, d=16, attn=3, act="idd", B=12, n_del=1, seed=21),      # 6 of 12 reached
    "e300_L3": dict(n_ent=300, n_rel=7, n_tri=3000, L=3, d=20, attn=5, act="tanh", B=12, n_del=40, seed=22),    # 8 of 12
    "e60_L2": dict(n_ent=60, n_rel=4, n_tri=150, L=2, d=16, attn=5, act="relu", B=20, n_del=1, seed=13),        # 8 of 20
    "e60_L3": dict(n_ent=60, n_rel=4, n_tri=150, L=3, d=16, attn=3, act="relu", B=20, n_del=3, seed=14),        # 7 of 20
}
