"""RED_GNN_trans.explain on the MI355X (-m gpu): the r-digraph of (s, r, o) and its attention, against the reference's own per-hop
edges and hidden states (tiny_fwd.npz), against the float64 oracle on real and synthetic KGs, and its properties."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import redgnn_oracle as orc
from tests import _util as U
from tests import explain_ref as X

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5


class P:
    def __init__(self, n_layer, hidden_dim, attn_dim, n_rel, act, dropout=0.0):
        self.n_layer, self.hidden_dim, self.attn_dim, self.n_rel, self.act, self.dropout = n_layer, hidden_dim, attn_dim, n_rel, act, dropout


def _loader(ids):
    from red_gnn_amd.load_data import DataLoader
    return DataLoader(ids=ids, verbose=False)


def _model(loader, n_layer, d, a, act, seed=1234, cls=None):
    from red_gnn_amd.models import RED_GNN_trans
    torch.manual_seed(seed)
    return (cls or RED_GNN_trans)(P(n_layer, d, a, loader.n_rel, act), loader).cuda().eval()


def _synthetic(n_ent=300, n_rel=7, n_tri=3000, seed=3):
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(n_ent, n_rel, n_tri, seed=seed)
    return dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)


def _rows(last_nodes, n_q, n_ent, rng, per_query=None, extra=2):
    """(query index, answer) rows: entities of each query's last level (all, or per_query of them) plus `extra` that are not in it."""
    q_of, objs = [], []
    for q in range(n_q):
        inside = last_nodes[last_nodes[:, 0] == q, 1]
        if per_query is not None and len(inside) > per_query:
            inside = rng.choice(inside, per_query, replace=False)
        outside = np.setdiff1d(np.arange(n_ent), last_nodes[last_nodes[:, 0] == q, 1])
        out = rng.choice(outside, min(extra, len(outside)), replace=False) if len(outside) else []
        for o in list(inside) + list(out):
            q_of.append(q)
            objs.append(int(o))
    return np.array(q_of), np.array(objs)


def _check_against(rd, exp, what=""):
    edges, alpha, offsets, reached = exp
    got = rd.edges.cpu().numpy()
    assert got.shape == edges.shape, (what, got.shape, edges.shape)
    assert np.array_equal(got, edges), what
    assert np.array_equal(rd.offsets.cpu().numpy(), offsets), what
    assert np.array_equal(rd.reached.cpu().numpy(), reached), what
    np.testing.assert_allclose(rd.alpha.cpu().numpy(), alpha, rtol=RTOL, atol=ATOL, err_msg=what)


def _oracle_case(model, og, graph, subs, rels, q_of, objs, n_layer, act, taus=(0.0,), mode="test"):
    """explain vs the float64 oracle's per-hop edges and alpha (trace).  tau = 0: the oracle's alpha decides nothing; tau > 0: the
    threshold is applied to the device's alpha of the tau = 0 digraph (same edges, same order), so that alphas within rounding of tau
    cannot flip the comparison."""
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    trace = []
    orc.forward(p, og, subs, rels, n_layer, act=act, dtype=torch.float64, trace=trace)
    hop_edges = X.expand_rows([t["edges"] for t in trace], q_of)
    hop_alpha = X.expand_alpha([t["edges"] for t in trace], [t["alpha"].numpy() for t in trace], q_of)
    last = trace[-1]["nodes"]
    last_rows = np.concatenate([np.stack([np.full((last[:, 0] == q).sum(), i), last[last[:, 0] == q, 1]], 1)
                                for i, q in enumerate(q_of)], 0)
    exp = X.expected_digraph(hop_edges, hop_alpha, objs, last_rows, 0.0, og.n_ent, graph)
    rd0 = model.explain(subs[q_of], rels[q_of], objs, mode=mode)
    _check_against(rd0, exp, "tau=0")
    e0 = rd0.edges.cpu().numpy()
    a0 = rd0.alpha.cpu().numpy()
    for tau in taus:
        if tau == 0.0:
            continue
        ok = X.rdigraph_mask(e0[:, 0], e0[:, 1], e0[:, 2], e0[:, 4], a0, objs, rd0.reached.cpu().numpy(), tau, og.n_ent, n_layer)
        rd = model.explain(subs[q_of], rels[q_of], objs, mode=mode, min_alpha=tau)
        assert np.array_equal(rd.edges.cpu().numpy(), e0[ok]), tau
        assert np.array_equal(rd.alpha.cpu().numpy(), a0[ok]), tau
        assert (rd.alpha.cpu().numpy() >= tau).all()
    return rd0


def test_tiny_fixture_pinned_to_the_reference():
    """tiny_fwd.npz: the reference's own per-hop edges, hidden states and parameters -> the r-digraph of every fixture query x every
    entity of its last level (and some outside it), alpha in float64 numpy."""
    from red_gnn_amd.models import RED_GNN_trans
    fx = U.load("tiny_fwd.npz")
    loader = _loader(fx)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    act = str(fx["act"])
    model = RED_GNN_trans(P(n_layer, d, a, loader.n_rel, act), loader).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    prm = U.params_of(fx)
    subs, rels = fx["subs"].astype(np.int64), fx["rels"].astype(np.int64)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))
    hop_alpha = []
    for l in range(n_layer):
        g = lambda k: prm["gnn_layers.%d.%s" % (l, k)].astype(np.float64)
        e = fx["L%d_edges" % l].astype(np.int64)
        hidden = np.zeros((len(subs), d)) if l == 0 else fx["L%d_hidden" % (l - 1)].astype(np.float64)
        rela = g("rela_embed.weight")
        pre = hidden[e[:, 4]] @ g("Ws_attn.weight").T + rela[e[:, 2]] @ g("Wr_attn.weight").T \
            + rela[rels[e[:, 0]]] @ g("Wqr_attn.weight").T + g("Wqr_attn.bias")
        hop_alpha.append(sig(np.maximum(pre, 0) @ g("w_alpha.weight").T + g("w_alpha.bias")).reshape(-1))
    last = fx["L%d_nodes" % (n_layer - 1)]
    q_of, objs = _rows(last, len(subs), int(fx["n_ent"]), np.random.default_rng(0), extra=3)
    hop_edges = X.expand_rows([fx["L%d_edges" % l] for l in range(n_layer)], q_of)
    hop_a = X.expand_alpha([fx["L%d_edges" % l] for l in range(n_layer)], hop_alpha, q_of)
    last_rows = np.concatenate([np.stack([np.full((last[:, 0] == q).sum(), i), last[last[:, 0] == q, 1]], 1) for i, q in enumerate(q_of)])
    graph = loader.graph_for("test")
    exp = X.expected_digraph(hop_edges, hop_a, objs, last_rows, 0.0, graph.n_ent, graph)
    rd = model.explain(subs[q_of], rels[q_of], objs, mode="test")
    _check_against(rd, exp, "tiny")
    # the score of o is the forward's, bit for bit
    with torch.no_grad():
        s = model(subs[q_of], rels[q_of], mode="test")
    assert torch.equal(rd.score, s[torch.arange(len(objs), device="cuda"), torch.as_tensor(objs, device="cuda")])


@pytest.mark.parametrize("d,a,act,n_layer", [(16, 3, "idd", 2), (20, 5, "tanh", 3), (32, 5, "relu", 3), (64, 5, "relu", 3),
                                            (128, 10, "relu", 2), (30, 30, "tanh", 2), (256, 5, "relu", 2), (100, 12, "tanh", 2),
                                            (48, 20, "relu", 2), (64, 27, "tanh", 2), (32, 17, "idd", 2)])
def test_explain_vs_oracle_widths(d, a, act, n_layer):
    """The widths of test_forward_vs_oracle_dims (fused and non-fused dense paths, attn > 16), tau in {0, 0.3, 0.6}."""
    ids = _synthetic()
    loader = _loader(ids)
    model = _model(loader, n_layer, d, a, act)
    rng = np.random.default_rng(0)
    subs, rels = rng.integers(0, ids["n_ent"], 5), rng.integers(0, 2 * ids["n_rel"], 5)
    og = U.oracle_graph(ids, "test")
    nodes = np.stack([np.arange(5), subs], 1)
    for _ in range(n_layer):
        nodes, _, _ = orc.get_neighbors(og, nodes)
    q_of, objs = _rows(nodes, 5, ids["n_ent"], rng, per_query=6)
    _oracle_case(model, og, loader.graph_for("test"), subs, rels, q_of, objs, n_layer, act, taus=(0.0, 0.3, 0.6))


@pytest.mark.parametrize("n_layer", [2, 3, 4, 5])
@pytest.mark.parametrize("ids_name", ["family_ids.npz", "umls_ids.npz", None])
def test_explain_vs_oracle_depths_and_kgs(n_layer, ids_name):
    ids = U.load(ids_name) if ids_name else _synthetic(200, 5, 1200, seed=n_layer)
    loader = _loader(ids)
    model = _model(loader, n_layer, 48, 5, "relu", seed=n_layer)
    rng = np.random.default_rng(n_layer)
    n_q = 8
    test = np.asarray(ids["test"])
    subs, rels = test[:n_q, 0].astype(np.int64), test[:n_q, 1].astype(np.int64)
    og = U.oracle_graph(ids, "test")
    nodes = np.stack([np.arange(n_q), subs], 1)
    for _ in range(n_layer):
        nodes, _, _ = orc.get_neighbors(og, nodes)
    q_of, objs = _rows(nodes, n_q, int(ids["n_ent"]), rng, per_query=7, extra=1)      # 64 rows
    _oracle_case(model, og, loader.graph_for("test"), subs, rels, q_of, objs, n_layer, "relu", taus=(0.0, 0.3, 0.6))


@pytest.mark.parametrize("mode", ["transductive", "inductive"])
def test_explain_inductive_loader(mode):
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    fx, ids = U.load("ind_WN18RR_v1_%s.npz" % mode), U.load("ind_WN18RR_v1_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    act = str(fx["act"])
    model = RED_GNN_induc(P(n_layer, d, a, loader.n_rel, act), loader).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    subs, rels = fx["subs"].astype(np.int64), fx["rels"].astype(np.int64)
    graph = loader.graph_for(mode)
    _, _, ip, ihr = graph.export()
    n_ent = graph.n_ent
    # the oracle graph of this mode from the device graph's own rows (add_inverse=False: the loader's triples are used as given)
    heads = ihr[:, 0].astype(np.int64)
    tails = np.repeat(np.arange(n_ent), np.diff(ip))
    kg = np.stack([heads, ihr[:, 1].astype(np.int64), tails], 1)
    kg = kg[kg[:, 1] != 2 * loader.n_rel]
    og = orc.OracleGraph(kg, n_ent, loader.n_rel)
    nodes = np.stack([np.arange(len(subs)), subs], 1)
    for _ in range(n_layer):
        nodes, _, _ = orc.get_neighbors(og, nodes)
    q_of, objs = _rows(nodes, len(subs), n_ent, np.random.default_rng(5), per_query=5, extra=1)
    # (the CSR order by tail does not depend on the fact-row order of other tails: the oracle graph's row order only has to keep the
    # device graph's order inside every tail, which the reconstruction above does)
    _oracle_case(model, og, graph, subs, rels, q_of, objs, n_layer, act, taus=(0.0, 0.3), mode=mode)
    with torch.no_grad():
        s = model(subs[q_of], rels[q_of], mode=mode)
    rd = model.explain(subs[q_of], rels[q_of], objs, mode=mode)
    assert torch.equal(rd.score, s[torch.arange(len(objs), device="cuda"), torch.as_tensor(objs, device="cuda")])


@pytest.mark.parametrize("d,a,act", [(48, 5, "relu"), (30, 30, "tanh")])
def test_faithfulness_score_depends_only_on_the_digraph(d, a, act):
    """The oracle's layer loop in float64 with every hop's edges restricted to the returned digraph gives the same score of o: the
    extracted digraph is everything the score depends on (identity edges carry the GRU state)."""
    ids = _synthetic(250, 6, 2500, seed=11)
    loader = _loader(ids)
    n_layer = 3
    model = _model(loader, n_layer, d, a, act, seed=7)
    og = U.oracle_graph(ids, "test")
    rng = np.random.default_rng(1)
    subs, rels = rng.integers(0, ids["n_ent"], 4), rng.integers(0, 2 * ids["n_rel"], 4)
    nodes = np.stack([np.arange(4), subs], 1)
    for _ in range(n_layer):
        nodes, _, _ = orc.get_neighbors(og, nodes)
    q_of, objs = _rows(nodes, 4, ids["n_ent"], rng, per_query=5, extra=0)
    rd = model.explain(subs[q_of], rels[q_of], objs, mode="test")
    e = rd.edges.cpu().numpy().astype(np.int64)
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    full = orc.forward(p, og, subs[q_of], rels[q_of], n_layer, act=act, dtype=torch.float64).numpy()
    actf = orc._ACTS[act]
    n = len(q_of)
    dd = p["W_final.weight"].shape[1]
    h0 = torch.zeros(n, dd, dtype=torch.float64)
    hidden = torch.zeros(n, dd, dtype=torch.float64)
    cur = np.stack([np.arange(n), subs[q_of]], 1)
    for l in range(n_layer):
        cur, edges, old_new = orc.get_neighbors(og, cur)
        key = lambda b, h, r, t: ((b * og.n_ent + h) * (2 * og.n_rel + 1) + r) * og.n_ent + t
        sel = e[e[:, 1] == l + 1]
        keep = np.isin(key(edges[:, 0], edges[:, 1], edges[:, 2], edges[:, 3]), key(sel[:, 0], sel[:, 2], sel[:, 3], sel[:, 4]))
        hidden, _, _ = orc.gnn_layer_forward(p, "gnn_layers.%d." % l, rels[q_of], hidden, edges[keep], len(cur), actf, torch.float64)
        h0n = torch.zeros(len(cur), dd, dtype=torch.float64)
        h0n[torch.as_tensor(old_new)] = h0
        hidden = orc.gru_step(p, hidden, h0n, torch.float64)
        h0 = hidden
    scores = (hidden @ p["W_final.weight"].double().T)[:, 0].numpy()
    idx = {(int(b), int(t)): i for i, (b, t) in enumerate(cur)}
    for i in range(n):
        ref = full[i, objs[i]]
        got = scores[idx[(i, int(objs[i]))]]
        assert abs(got - ref) <= 1e-12 * max(abs(ref), 1e-300), (i, got, ref)


def test_properties_unreached_argmax_batch_invariance_determinism():
    ids = _synthetic(300, 7, 400, seed=3)          # sparse: two hops leave most entities unvisited
    loader = _loader(ids)
    model = _model(loader, 2, 32, 5, "relu")
    rng = np.random.default_rng(4)
    n = 24
    subs, rels = rng.integers(0, ids["n_ent"], n), rng.integers(0, 2 * ids["n_rel"], n)
    objs = rng.integers(0, ids["n_ent"], n)
    trace = []
    with torch.no_grad():
        model(subs, rels, mode="test", trace=trace)
    last = trace[-1]["nodes"].cpu().numpy()
    for b in range(0, n, 2):                       # half the rows with an answer inside the last level
        objs[b] = rng.choice(last[last[:, 0] == b, 1])
    was_training = model.training
    rd = model.explain(subs, rels, objs)
    assert model.training == was_training
    with torch.no_grad():
        s = model(subs, rels, mode="test")
    ar = torch.arange(n, device="cuda")
    assert torch.equal(rd.score, s[ar, torch.as_tensor(objs, device="cuda")])
    off = rd.offsets.cpu().numpy()
    reached = rd.reached.cpu().numpy()
    assert (~reached).sum() > 0 and reached.sum() > 0
    for b in np.nonzero(~reached)[0]:
        assert off[b + 1] == off[b] and rd.score[b].item() == 0.0
    # objs=None == the argmax
    rd_top = model.explain(subs, rels)
    rd_arg = model.explain(subs, rels, s.argmax(1).cpu().numpy())
    for f in ("edges", "alpha", "offsets", "reached", "score"):
        assert torch.equal(getattr(rd_top, f), getattr(rd_arg, f)), f
    # a second call equals the first; each row alone equals its slice of the batch
    rd2 = model.explain(subs, rels, objs)
    for f in ("edges", "alpha", "offsets", "reached", "score"):
        assert torch.equal(getattr(rd, f), getattr(rd2, f)), f
    for b in range(0, n, 5):
        one = model.explain(subs[b:b + 1], rels[b:b + 1], objs[b:b + 1])
        sl = slice(off[b], off[b + 1])
        e = rd.edges[sl].clone()
        e[:, 0] = 0
        assert torch.equal(one.edges, e) and torch.equal(one.alpha, rd.alpha[sl])
        assert torch.equal(one.score[0], rd.score[b]) and bool(one.reached[0]) == bool(reached[b])
    # training mode with dropout: explain still has eval semantics and leaves the flag alone
    model.dropout.p = 0.5
    model.train()
    rd3 = model.explain(subs, rels, objs)
    assert model.training
    model.eval()
    for f in ("edges", "alpha", "offsets", "reached"):
        assert torch.equal(getattr(rd, f), getattr(rd3, f)), f
    # strongest paths lie in the digraph and run s -> o
    rl, en, pr = rd.strongest_paths()
    for b in np.nonzero(reached)[0]:
        if off[b + 1] == off[b]:
            continue
        assert en[b, 0].item() == subs[b] and en[b, -1].item() == objs[b] and pr[b].item() > 0


def test_ids_are_validated_like_forward():
    ids = _synthetic()
    loader = _loader(ids)
    model = _model(loader, 2, 16, 3, "idd")
    with pytest.raises(ValueError):
        model.explain([ids["n_ent"]], [0], [0])
    with pytest.raises(ValueError):
        model.explain([0], [2 * ids["n_rel"] + 1], [0])
    with pytest.raises(ValueError):
        model.explain([0], [0], [ids["n_ent"]])
    with pytest.raises(ValueError):
        model.explain([0], [0], [-1])


def test_argument_errors_with_a_frontier():
    from red_gnn_amd import _lib, engine
    ids = _synthetic()
    loader = _loader(ids)
    graph = loader.graph_for("test")
    fr = engine.Frontier(graph.n_ent, 4, 3)
    fr.reset(torch.zeros(4, dtype=torch.int32, device="cuda"))
    fr.expand(graph)
    L = _lib.lib()
    objs = torch.zeros(4, dtype=torch.int32, device="cuda")
    marks = torch.zeros((4, (graph.n_ent + 31) // 32), dtype=torch.int32, device="cuda")
    reached = torch.zeros(4, dtype=torch.bool, device="cuda")
    s = _lib.stream_ptr()
    assert L.rg_explain_seed(fr.handle, 4, graph.n_ent, 2, _lib.ptr(objs), _lib.ptr(marks), _lib.ptr(reached), s) != 0
    assert b"not resident" in L.rg_last_error()
    assert L.rg_explain_seed(fr.handle, 5, graph.n_ent, 1, _lib.ptr(objs), _lib.ptr(marks), _lib.ptr(reached), s) != 0
    assert b"frontier has batch" in L.rg_last_error()
    f32 = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    wp = torch.zeros(marks.numel() + 1, dtype=torch.int32, device="cuda")
    n_e = C.c_int64()
    for level, batch, n_ent, msg in ((2, 4, graph.n_ent, b"not resident"), (1, 4, graph.n_ent + 1, b"frontier has batch")):
        assert L.rg_explain_count(fr.handle, graph.handle, batch, n_ent, level, _lib.ptr(marks), _lib.ptr(f32), _lib.ptr(f32),
                                  _lib.ptr(f32), 4, _lib.ptr(f32), _lib.ptr(f32), 3, 0.0, _lib.ptr(marks), _lib.ptr(wp), None, 0,
                                  C.byref(n_e), s) != 0
        assert msg in L.rg_last_error()
    assert engine.explain_seed(fr, 1, objs)[1].all()        # entity 0 is the start node of every row: in level 1 (identity edge)


def test_c2_shape_scale():
    """C2 (10 k entities / 200 k triples) at B = 64: hop-1 heads are s, hop-L tails are o, per-hop counts within the subgraph's."""
    from red_gnn_amd.synthetic import make_shape
    kg = make_shape("C2")
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = _loader(ids)
    model = _model(loader, 3, 64, 5, "relu")
    subs, rels = kg.test[:64, 0], kg.test[:64, 1]
    rd = model.explain(subs, rels)                 # the model's top answers: all reached
    sub_edges = model.last_stats["n_edges"]
    e = rd.edges.cpu().numpy()
    assert rd.reached.any()
    with torch.no_grad():
        s = model(subs, rels, mode="test")
    top = s.argmax(1).cpu().numpy()
    h1 = e[e[:, 1] == 1]
    assert np.array_equal(h1[:, 2], np.asarray(subs)[h1[:, 0]])
    hL = e[e[:, 1] == 3]
    assert np.array_equal(hL[:, 4], top[hL[:, 0]])
    for l in range(1, 4):
        assert (e[:, 1] == l).sum() <= sub_edges[l - 1]
    al = rd.alpha.cpu().numpy()
    assert ((al >= 0) & (al <= 1)).all()
    assert len(e) > 0
