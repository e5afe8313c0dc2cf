"""RED_GNN_trans.attention_profile on the MI355X (-m gpu): counts and alpha sums per (query | query relation, hop, edge relation)
against the reference's own per-hop edges (tiny_fwd.npz), against the float64 oracle on real and synthetic KGs, against explain, and
the bit-for-bit properties of the integer sums.

Tolerance.  Counts are exact everywhere.  A sum carries the per-alpha tolerance of tests/test_explain_gpu.py (device alpha against
the float64 oracle: RTOL, ATOL = 1e-4, 1e-5) through the sum, plus the kernel's stated per-edge rounding Q = 2^-33:
|sum_dev - sum_ref| <= RTOL * sum_ref + (ATOL + Q) * count per cell."""
import numpy as np
import pytest
import torch

from oracle import redgnn_oracle as orc
from tests import _util as U
from tests import profile_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
Q = 2.0 ** -33


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


def _same(p1, p2):
    return torch.equal(p1.count, p2.count) and torch.equal(p1.fixed, p2.fixed) and torch.equal(p1.alpha_sum, p2.alpha_sum)


def _check(prof, count_ref, sum_ref, what=""):
    count, asum = prof.count.cpu().numpy(), prof.alpha_sum.cpu().numpy()
    assert count.shape == count_ref.shape and count.dtype == np.int64 and asum.dtype == np.float64, (what, count.shape, count_ref.shape)
    assert np.array_equal(count, count_ref), what
    err = np.abs(asum - sum_ref)
    bound = RTOL * sum_ref + (ATOL + Q) * count_ref
    worst = float((err - bound).max())
    print("%s: cells with edges %d, largest |sum error| %.3g, largest error / bound %.3g"
          % (what, int((count_ref > 0).sum()), float(err.max()), float((err / np.maximum(bound, 1e-300))[count_ref > 0].max(initial=0.0))))
    assert worst <= 0.0, (what, worst)
    assert (asum[count_ref == 0] == 0.0).all(), what


def _against(model, subs, rels, hop_edges, hop_alpha, mode="test", what=""):
    n_rows = 2 * model.n_rel + 1
    count, asum = R.profile_by_query(hop_edges, hop_alpha, len(subs), n_rows)
    pq = model.attention_profile(subs, rels, mode=mode, group="query")
    assert pq.group == "query" and pq.count.is_cuda
    _check(pq, count, asum, what + " group=query")
    pr = model.attention_profile(subs, rels, mode=mode, group="relation")
    _check(pr, *R.by_relation(count, asum, rels, n_rows), what + " group=relation")
    return pq, pr


def _oracle_case(model, og, subs, rels, n_layer, act, mode="test", what=""):
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    trace = []
    orc.forward(p, og, subs, rels, n_layer, act=act, dtype=torch.float64, trace=trace)
    return _against(model, subs, rels, [t["edges"] for t in trace], [t["alpha"].numpy().reshape(-1) for t in trace], mode, what)


def test_tiny_fixture_pinned_to_the_reference():
    """tiny_fwd.npz: the reference's own per-hop edges, hidden states and parameters; alpha in float64 numpy from them."""
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
    _against(model, subs, rels, [fx["L%d_edges" % l] for l in range(n_layer)], hop_alpha, what="tiny")


@pytest.mark.parametrize("d,a,act,n_layer", [(16, 3, "idd", 2), (20, 5, "tanh", 3), (32, 5, "relu", 3), (64, 5, "relu", 3),
                                            (128, 10, "relu", 2), (30, 30, "tanh", 2), (256, 5, "relu", 2), (100, 12, "tanh", 2),
                                            (48, 20, "relu", 2), (64, 27, "tanh", 2), (32, 17, "idd", 2)])
def test_profile_vs_oracle_widths(d, a, act, n_layer):
    """The widths and activations of test_explain_vs_oracle_widths (fused and non-fused dense paths, attn > 16)."""
    ids = _synthetic()
    loader = _loader(ids)
    model = _model(loader, n_layer, d, a, act)
    rng = np.random.default_rng(0)
    subs, rels = rng.integers(0, ids["n_ent"], 5), rng.integers(0, 2 * ids["n_rel"], 5)
    _oracle_case(model, U.oracle_graph(ids, "test"), subs, rels, n_layer, act, what="d=%d a=%d %s" % (d, a, act))


@pytest.mark.parametrize("n_layer", [2, 3, 4, 5])
@pytest.mark.parametrize("ids_name", ["family_ids.npz", "umls_ids.npz", None])
def test_profile_vs_oracle_depths_and_kgs(n_layer, ids_name):
    ids = U.load(ids_name) if ids_name else _synthetic(200, 5, 1200, seed=n_layer)
    loader = _loader(ids)
    model = _model(loader, n_layer, 48, 5, "relu", seed=n_layer)
    test = np.asarray(ids["test"])
    subs, rels = test[:8, 0].astype(np.int64), test[:8, 1].astype(np.int64)
    _oracle_case(model, U.oracle_graph(ids, "test"), subs, rels, n_layer, "relu", what="%s L=%d" % (ids_name, n_layer))


@pytest.mark.parametrize("mode", ["transductive", "inductive"])
def test_profile_inductive_loader(mode):
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
    # the oracle graph of this mode from the device graph's own rows, as tests/test_explain_gpu.py builds it
    kg = np.stack([ihr[:, 0].astype(np.int64), ihr[:, 1].astype(np.int64), np.repeat(np.arange(n_ent), np.diff(ip))], 1)
    kg = kg[kg[:, 1] != 2 * loader.n_rel]
    og = orc.OracleGraph(kg, n_ent, loader.n_rel)
    _oracle_case(model, og, subs, rels, n_layer, act, mode=mode, what="inductive loader, %s" % mode)
    if mode == "transductive":                               # RED_GNN_induc's default mode
        assert _same(model.attention_profile(subs, rels), model.attention_profile(subs, rels, mode="transductive"))


def test_repeated_queries_and_relations():
    ids = _synthetic(250, 6, 2500, seed=11)
    loader = _loader(ids)
    model = _model(loader, 3, 32, 5, "relu", seed=7)
    subs = np.array([5, 5, 17, 5, 40, 17, 5, 99, 40, 5])
    rels = np.array([2, 2, 2, 9, 9, 2, 2, 0, 9, 3])          # rows 0, 1, 6 are the same query; relation 2 and 9 asked five / three times
    pq, pr = _oracle_case(model, U.oracle_graph(ids, "test"), subs, rels, 3, "relu", what="repeated")
    assert torch.equal(pq.count[0], pq.count[1]) and torch.equal(pq.fixed[0], pq.fixed[6])
    asked = np.unique(rels)
    rest = np.setdiff1d(np.arange(13), asked)
    assert not pr.count[torch.as_tensor(rest, device="cuda")].any() and pr.count[torch.as_tensor(asked, device="cuda")].any()


def test_many_relations_take_the_global_bins():
    """2 * 1500 + 1 relation rows with 8 attention columns: 132 KB of table and bins, above the 48 KB a workgroup keeps in LDS, so the
    kernel adds into the output buffers directly.  Same checks, and the split / permutation properties."""
    ids = _synthetic(120, 1500, 2500, seed=5)
    loader = _loader(ids)
    model = _model(loader, 3, 16, 5, "relu", seed=3)
    rng = np.random.default_rng(2)
    subs, rels = rng.integers(0, ids["n_ent"], 6), rng.integers(0, 2 * ids["n_rel"], 6)
    pq, pr = _oracle_case(model, U.oracle_graph(ids, "test"), subs, rels, 3, "relu", what="3001 relation rows")
    assert _same(pr, model.attention_profile(subs[:2], rels[:2]) + model.attention_profile(subs[2:], rels[2:]))
    perm = rng.permutation(6)
    assert torch.equal(model.attention_profile(subs[perm], rels[perm], group="query").fixed, pq.fixed[torch.as_tensor(perm, device="cuda")])


def test_properties_bit_for_bit():
    ids = _synthetic(300, 7, 3000, seed=3)
    loader = _loader(ids)
    model = _model(loader, 3, 32, 5, "relu")
    rng = np.random.default_rng(4)
    n = 24
    subs, rels = rng.integers(0, ids["n_ent"], n), rng.integers(0, 2 * ids["n_rel"], n)
    n_rows = 2 * ids["n_rel"] + 1
    with torch.no_grad():
        before = model(subs, rels, mode="test")
        edges_fwd = list(model.last_stats["n_edges"])
    was_training = model.training
    pr = model.attention_profile(subs, rels)
    pq = model.attention_profile(subs, rels, group="query")
    assert model.training == was_training
    assert pr.count.shape == (n_rows, 3, n_rows) and pq.count.shape == (n, 3, n_rows)
    assert pr.alpha_sum.dtype == torch.float64 and pr.count.dtype == torch.int64
    # two runs equal
    assert _same(pr, model.attention_profile(subs, rels)) and _same(pq, model.attention_profile(subs, rels, group="query"))
    # halves and singletons sum to the whole
    half = model.attention_profile(subs[:n // 2], rels[:n // 2]) + model.attention_profile(subs[n // 2:], rels[n // 2:])
    assert _same(pr, half)
    ones = None
    for b in range(n):
        one = model.attention_profile(subs[b:b + 1], rels[b:b + 1])
        ones = one if ones is None else ones + one
        single = model.attention_profile(subs[b:b + 1], rels[b:b + 1], group="query")
        assert torch.equal(single.fixed[0], pq.fixed[b]) and torch.equal(single.count[0], pq.count[b])
    assert _same(pr, ones)
    # a permutation of the queries: the same relation table, the permuted query rows
    perm = rng.permutation(n)
    assert _same(pr, model.attention_profile(subs[perm], rels[perm]))
    pp = model.attention_profile(subs[perm], rels[perm], group="query")
    perm_t = torch.as_tensor(perm, device="cuda")
    assert torch.equal(pp.fixed, pq.fixed[perm_t]) and torch.equal(pp.count, pq.count[perm_t])
    # group="relation" == the integer index_add of group="query" by rels
    rels_t = torch.as_tensor(rels, device="cuda")
    assert torch.equal(pr.fixed, torch.zeros_like(pr.fixed).index_add_(0, rels_t, pq.fixed))
    assert torch.equal(pr.count, torch.zeros_like(pr.count).index_add_(0, rels_t, pq.count))
    assert torch.equal(pr.alpha_sum, pr.fixed.double() * 2.0 ** -32)
    # the edges are the forward's
    assert pq.count.sum((0, 2)).tolist() == edges_fwd and pr.count.sum((0, 2)).tolist() == edges_fwd
    # sums lie in [0, count]; the mean is NaN exactly where there is no edge
    assert (pr.fixed >= 0).all() and (pr.alpha_sum <= pr.count.double()).all()
    assert torch.equal(torch.isnan(pr.mean()), pr.count == 0)
    # a forward after the profile is the forward without it - eagerly, and once the forward is a replayed graph
    with torch.no_grad():
        assert torch.equal(model(subs, rels, mode="test"), before)
        replayed = [model(subs, rels, mode="test") for _ in range(3)][-1]
        assert _same(pr, model.attention_profile(subs, rels))
        assert torch.equal(model(subs, rels, mode="test"), replayed)
        assert list(model.last_stats["n_edges"]) == edges_fwd
    # training mode with dropout: eval semantics, the flag is left alone
    model.dropout.p = 0.5
    model.train()
    p3 = model.attention_profile(subs, rels)
    assert model.training
    model.eval()
    assert _same(pr, p3)


def test_ids_are_validated_like_explain():
    ids = _synthetic()
    loader = _loader(ids)
    model = _model(loader, 2, 16, 3, "idd")
    for subs, rels, msg in (([ids["n_ent"]], [0], "out of range"), ([0], [2 * ids["n_rel"] + 1], "out of range"), ([-1], [0], "out of range"),
                            ([0, 1], [0], "one relation per subject"), ([], [], "one relation per subject")):
        with pytest.raises(ValueError, match=msg):
            model.attention_profile(subs, rels)
    with pytest.raises(ValueError, match="group"):
        model.attention_profile([0], [0], group="entity")
    assert model.attention_profile([0], [2 * ids["n_rel"]]).count.sum() > 0     # the identity relation is a valid query relation


def test_argument_errors_with_a_frontier():
    from red_gnn_amd import _lib, engine
    ids = _synthetic()
    loader = _loader(ids)
    graph = loader.graph_for("test")
    fr = engine.Frontier(graph.n_ent, 4, 3)
    fr.reset(torch.zeros(4, dtype=torch.int32, device="cuda"))
    fr.expand(graph)
    L = _lib.lib()
    n_rows = 2 * ids["n_rel"] + 1
    f32 = torch.zeros((max(4, n_rows), 4), dtype=torch.float32, device="cuda")
    out = torch.zeros((4, n_rows), dtype=torch.int64, device="cuda")
    s = _lib.stream_ptr()

    def call(batch=4, n_ent=graph.n_ent, level=1, n_old=4):
        return L.rg_attn_profile(fr.handle, graph.handle, batch, n_ent, level, n_old, _lib.ptr(f32), _lib.ptr(f32), _lib.ptr(f32), 4,
                                 _lib.ptr(f32), _lib.ptr(f32), 3, _lib.ptr(out), _lib.ptr(out), s)

    for kw, msg in ((dict(level=2), b"not resident"), (dict(batch=5), b"frontier has batch"), (dict(n_ent=graph.n_ent + 1), b"frontier has batch"),
                    (dict(n_old=5), b"n_old=5")):
        assert call(**kw) != 0, kw
        assert msg in L.rg_last_error(), (kw, L.rg_last_error())
    assert call() == 0
    torch.cuda.synchronize()
    assert out.sum().item() > 0


def test_consistent_with_explain():
    """explain with objs ranging over every entity of a query's last level returns each hop-L edge of that query in exactly one answer's
    digraph: grouped by relation those rows are the profile's hop-L cells - counts exactly, float alphas summed in float64 within
    Q * count."""
    ids = _synthetic(200, 5, 1200, seed=2)
    loader = _loader(ids)
    L = 3
    model = _model(loader, L, 32, 5, "relu", seed=5)
    n_rows = 2 * ids["n_rel"] + 1
    for s, r in ((3, 1), (150, 7)):
        trace = []
        with torch.no_grad():
            model(np.array([s]), np.array([r]), mode="test", trace=trace)
        last = trace[-1]["nodes"].cpu().numpy()[:, 1]
        rd = model.explain(np.full(len(last), s), np.full(len(last), r), last)
        e = rd.edges.cpu().numpy()
        a = rd.alpha.cpu().numpy().astype(np.float64)
        m = e[:, 1] == L
        count = np.bincount(e[m, 3], minlength=n_rows)
        asum = np.bincount(e[m, 3], weights=a[m], minlength=n_rows)
        pq = model.attention_profile([s], [r], group="query")
        assert np.array_equal(pq.count[0, L - 1].cpu().numpy(), count)
        err = np.abs(pq.alpha_sum[0, L - 1].cpu().numpy() - asum)
        print("explain vs profile: %d hop-%d edges, largest |sum error| %.3g (bound Q * count, largest %.3g)" % (m.sum(), L, err.max(), Q * count.max()))
        assert (err <= Q * count).all(), float((err - Q * count).max())


def test_base_model_whole_split():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(60, 4, 400, seed=2)
    loader = _loader(dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test))

    class Opt:
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch, n_tbatch = 0.01, 0.99, 1e-5, 16, 3, 2, 0.0, "relu", 8, 8
        n_rel = loader.n_rel

    bm = BaseModel(Opt, loader)
    for data, query in (("test", loader.test_q), ("valid", loader.valid_q)):
        assert len(query) > 8                                # more than one batch
        subs, rels = np.array([q[0] for q in query]), np.array([q[1] for q in query])
        whole = bm.attention_profile(data)
        parts = None
        for lo in range(0, len(query), 8):
            p = bm.model.attention_profile(subs[lo:lo + 8], rels[lo:lo + 8], mode=data)
            parts = p if parts is None else parts + p
        assert _same(whole, parts) and whole.group == "relation"
        assert _same(whole, bm.model.attention_profile(subs, rels, mode=data))      # ... and does not depend on n_tbatch
        first = bm.attention_profile(data, max_queries=5)
        assert _same(first, bm.model.attention_profile(subs[:5], rels[:5], mode=data))
    with pytest.raises(ValueError):
        bm.attention_profile("train")


def test_c2_shape_scale():
    """C2 (10 k entities / 200 k triples) at B = 64: per-hop counts equal the forward's edge counts, two runs equal, sums in [0, count]."""
    from red_gnn_amd.synthetic import make_shape
    kg = make_shape("C2")
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = _loader(ids)
    model = _model(loader, 3, 64, 5, "relu")
    subs, rels = kg.test[:64, 0], kg.test[:64, 1]
    with torch.no_grad():
        model(subs, rels, mode="test")
        edges_fwd = list(model.last_stats["n_edges"])
    pq = model.attention_profile(subs, rels, group="query")
    assert pq.count.sum((0, 2)).tolist() == edges_fwd
    assert _same(pq, model.attention_profile(subs, rels, group="query"))
    pr = model.attention_profile(subs, rels)
    assert pr.count.sum((0, 2)).tolist() == edges_fwd
    assert torch.equal(pr.count.sum(0), pq.count.sum(0)) and torch.equal(pr.fixed.sum(0), pq.fixed.sum(0))
    for p in (pq, pr):
        assert (p.fixed >= 0).all() and (p.alpha_sum <= p.count.double()).all()
    print("C2 B=64 edges per hop", edges_fwd)
