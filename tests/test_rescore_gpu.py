"""RDigraph.rescore, fact masks and model.fidelity on the MI355X (-m gpu): against the float64 numpy reference of tests/rescore_ref.py
(the oracle's arithmetic over the explicit edge list), against the model's own forward on a knowledge graph rebuilt without the deleted
facts, and the properties of the fidelity measures.  Tolerance: the project's stated one through tests/_util.assert_close_fp32, rtol 1e-4
and atol 2e-5 of the fp64 reference, or 4x the fp32 reference's own error."""
import numpy as np
import pytest
import torch

from oracle import redgnn_oracle as orc
from tests import _util as U
from tests import rescore_ref as R
from tests.test_explain_gpu import P, _loader, _model, _synthetic

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
N_ROWS = 12
# (d, attn, act, L); (32, 17, idd, 2) has no fused dense kernel (attn > 16): the tall_linear / gru_step path
CONFIGS = [(16, 3, "idd", 2), (20, 5, "tanh", 3), (64, 5, "relu", 3), (128, 10, "relu", 2), (32, 17, "idd", 2)]
# facts picked per row for deletion (their union is deleted for every row), chosen with the reference alone so that at least a quarter
# of the rows stay reached and at least one does not (asserted below): (n_del, seed) per L
PICK = {2: (1, 5), 3: (30, 5)}

_IDS = {}


def _ids():
    if not _IDS:
        _IDS.update(_synthetic())
    return _IDS


def rows_and_facts(ids, L, n_rows=N_ROWS):
    """(subs, rels, objs, facts): ``n_rows`` random queries with an answer drawn from their level-L set, and the union of PICK[L] facts
    picked from each row's digraph - all from the CPU oracle."""
    n_del, seed = PICK[L]
    rng = np.random.default_rng(seed)
    n_ent, n_rel = int(ids["n_ent"]), int(ids["n_rel"])
    og = U.oracle_graph(ids, "test")
    subs, rels = rng.integers(0, n_ent, n_rows), rng.integers(0, 2 * n_rel, n_rows)
    nodes, trace = np.stack([np.arange(n_rows), subs], 1), []
    for _ in range(L):
        nodes, edges, _ = orc.get_neighbors(og, nodes)
        trace.append(dict(nodes=nodes, edges=edges))
    objs = np.array([rng.choice(nodes[nodes[:, 0] == b, 1]) for b in range(n_rows)])
    edges, offsets, reached = R.digraph_of(trace, np.arange(n_rows), objs, n_ent)
    facts = set()
    for b in range(n_rows):
        mine = edges[offsets[b]:offsets[b + 1]]
        distinct = sorted({R.base_fact(h, r, t, n_rel) for _, _, h, r, t in mine.tolist() if r != 2 * n_rel})
        facts.update(distinct[j] for j in rng.permutation(len(distinct))[:n_del])
    return subs, rels, objs, np.array(sorted(facts), np.int64).reshape(-1, 3), edges


def _params(model):
    return {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}


def _compare(tag, rs, ref64, ref32):
    score, reached, live, alpha = ref64
    assert np.array_equal(rs.reached.cpu().numpy(), reached), tag + ": reached"
    assert np.array_equal(rs.live.cpu().numpy(), live), tag + ": live"
    got = rs.score.cpu().numpy()
    assert (got[~reached] == 0).all(), tag + ": an unreached row does not score exactly 0"
    print("%s: max |score - ref64| %.3g (ref32: %.3g), max |alpha - ref64| %.3g"
          % (tag, np.abs(got - score).max(), np.abs(ref32[0] - score).max(), np.abs(rs.alpha.cpu().numpy() - alpha).max()))
    U.assert_close_fp32(got, ref32[0], score, RTOL, ATOL, tag + " score")
    U.assert_close_fp32(rs.alpha.cpu().numpy(), ref32[3], alpha, RTOL, ATOL, tag + " alpha")
    assert (rs.alpha.cpu().numpy()[~live] == 0).all(), tag + ": a dead edge carries attention"


@pytest.mark.parametrize("d,a,act,L", CONFIGS)
def test_rescore_against_the_reference_and_the_rebuilt_graph(d, a, act, L):
    ids = _ids()
    loader = _loader(ids)
    model = _model(loader, L, d, a, act)
    n_ent, n_rel = loader.n_ent, loader.n_rel
    subs, rels, objs, facts, want_edges = rows_and_facts(ids, L)
    rd = model.explain(subs, rels, objs)
    e = rd.edges.cpu().numpy().astype(np.int64)
    assert np.array_equal(U.sorted_edges(e), U.sorted_edges(want_edges)) and bool(rd.reached.all())
    p = _params(model)
    ref = lambda keep, dt: R.rescore(p, e, subs, rels, n_ent, L, act, keep=keep, dtype=dt)
    tag = "d%d a%d %s L%d" % (d, a, act, L)

    # ---- every edge kept: the model's own score
    rs = rd.rescore(model)
    _compare(tag + " keep=None", rs, ref(None, np.float64), ref(None, np.float32))
    assert bool(rs.live.all()) and bool(rs.reached.all())
    np.testing.assert_allclose(rs.score.cpu().numpy(), rd.score.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)   # two fp32 evaluations
    again = rd.rescore(model, keep=torch.ones(len(e), dtype=torch.uint8, device="cuda"))
    assert torch.equal(again.score, rs.score) and torch.equal(again.alpha, rs.alpha)

    # ---- the facts deleted, in both directions and at every hop
    m = rd.fact_mask(facts)
    assert np.array_equal(m.cpu().numpy(), R.fact_mask(e, n_rel, facts))
    keep = ~m
    rs = rd.rescore(model, keep=keep)
    k_h = keep.cpu().numpy()
    assert torch.equal(rd.rescore(model, keep=k_h.astype(np.uint8)).score, rs.score)      # a host array goes along, bits unchanged
    r64, r32 = ref(k_h, np.float64), ref(k_h, np.float32)
    reached = r64[1]
    print("%s: %d facts deleted, %d of %d edges kept, %d live, %d of %d rows reached" % (tag, len(facts), k_h.sum(), len(e), r64[2].sum(),
                                                                                      reached.sum(), len(subs)))
    assert 4 * reached.sum() >= len(subs) and (~reached).any(), "the inputs must leave a quarter of the rows reached and cut one off"
    assert (k_h & ~r64[2]).any(), "the inputs must leave kept edges dangling"
    _compare(tag + " facts deleted", rs, r64, r32)

    # ---- ... is the model's forward on the knowledge graph without them
    cut = dict(ids)
    cut["facts"], cut["train"] = R.without_facts(ids["facts"], facts), R.without_facts(ids["train"], facts)
    assert len(cut["facts"]) + len(cut["train"]) < len(ids["facts"]) + len(ids["train"])
    model.loader = _loader(cut)
    try:
        with torch.no_grad():
            fwd = model(subs, rels, mode="test")[np.arange(len(subs)), objs].cpu().numpy()
    finally:
        model.loader = loader
    assert np.array_equal(fwd != 0, reached), tag + ": the forward on the rebuilt graph reaches other rows"
    U.assert_close_fp32(fwd, r32[0], r64[0], RTOL, ATOL, tag + " forward on the rebuilt graph")
    # (two fp32 evaluations of one number, each within the tolerance of it)
    np.testing.assert_allclose(rs.score.cpu().numpy(), fwd, rtol=2 * RTOL, atol=2 * ATOL)


@pytest.mark.parametrize("mode", ["transductive", "inductive"])
def test_rescore_inductive(mode):
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    fx, ids = U.load("ind_WN18RR_v1_%s.npz" % mode), U.load("ind_WN18RR_v1_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    act = str(fx["act"])
    model = RED_GNN_induc(P(n_layer, d, a, loader.n_rel, act), loader).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    subs, rels = fx["subs"].astype(np.int64)[:N_ROWS], fx["rels"].astype(np.int64)[:N_ROWS]
    n_ent = loader.graph_for(mode).n_ent
    rd = model.explain(subs, rels, mode=mode)                 # each row's own top answer
    e = rd.edges.cpu().numpy().astype(np.int64)
    p = _params(model)
    ref = lambda keep, dt: R.rescore(p, e, subs, rels, n_ent, n_layer, act, keep=keep, dtype=dt)
    _compare(mode + " keep=None", rd.rescore(model, mode=mode), ref(None, np.float64), ref(None, np.float32))
    paths = rd.top_paths(1)
    m = paths.fact_mask(1)
    assert np.array_equal(m.cpu().numpy(), R.fact_mask(e, loader.n_rel, e[paths.edge[paths.edge >= 0].cpu().numpy()][:, 2:5],
                                                       e[paths.edge[paths.edge >= 0].cpu().numpy()][:, 0]))
    k_h = (~m).cpu().numpy()
    _compare(mode + " best path deleted", rd.rescore(model, keep=~m, mode=mode), ref(k_h, np.float64), ref(k_h, np.float32))
    only = (m | (rd.edges[:, 3] == 2 * loader.n_rel))
    _compare(mode + " best path only", rd.rescore(model, keep=only, mode=mode), ref(only.cpu().numpy(), np.float64),
             ref(only.cpu().numpy(), np.float32))
    with pytest.raises(ValueError, match="out of range"):   # the other mode's graph has another entity count or the ids do not fit it
        bad = rd.edges.clone()
        bad[0, 4] = 10 ** 6
        type(rd)(**{**rd.__dict__, "edges": bad}).rescore(model, mode=mode)


def test_fidelity_columns_are_rescores_of_the_path_masks():
    ids = _ids()
    loader = _loader(ids)
    d, a, act, L = CONFIGS[0]
    k, B = 3, 2 * N_ROWS
    model = _model(loader, L, d, a, act)
    subs, rels, objs, _, _ = rows_and_facts(ids, L, n_rows=B)
    f = model.fidelity(subs, rels, objs, k=k)
    rd, paths = f.paths.digraph, f.paths
    assert f.score is rd.score and f.without.shape == f.only.shape == f.reached_without.shape == f.reached_only.shape == (B, k)
    assert torch.equal(f.count, paths.count) and paths.edge.shape[1] == k
    loops = rd.edges[:, 3] == 2 * loader.n_rel
    for j in range(k):
        m = paths.fact_mask(j + 1)
        wo, on = rd.rescore(model, keep=~m), rd.rescore(model, keep=m | loops)
        assert torch.equal(f.without[:, j], wo.score) and torch.equal(f.reached_without[:, j], wo.reached)
        assert torch.equal(f.only[:, j], on.score) and torch.equal(f.reached_only[:, j], on.reached)
    assert torch.equal(f.necessity(), f.score[:, None] - f.without) and torch.equal(f.sufficiency_gap(), f.score[:, None] - f.only)
    assert len(f.format()) == B
    count = f.count.cpu().numpy()
    rw = f.reached_without.cpu().numpy()
    print("paths per row %s; reached without the best j paths: %s of %d" % (count.tolist(), rw.sum(0).tolist(), B))
    # the inputs: both outcomes of the deletion occur, and some row has no more than k paths in all
    assert 4 * rw[:, 0].sum() >= B and (~rw).any()
    total = rd.top_paths(k + 1).count.cpu().numpy()
    few = np.nonzero((total <= k) & (total >= 1))[0]
    assert len(few) >= 1 and (count[few] == total[few]).all()
    # for j past count a row repeats its value at j = count
    for b in range(B):
        for j in range(max(count[b], 1), k):
            assert f.without[b, j] == f.without[b, count[b] - 1 if count[b] else 0] and f.only[b, j] == f.only[b, max(count[b] - 1, 0)]
    # a row whose digraph has at most k paths: those paths' facts and the self-loops are the whole digraph, ``only`` is the score
    e = rd.edges.cpu().numpy().astype(np.int64)
    p = _params(model)
    s64 = R.rescore(p, e, subs, rels, loader.n_ent, L, act)[0]
    s32 = R.rescore(p, e, subs, rels, loader.n_ent, L, act, dtype=np.float32)[0]
    only_at_count = f.only.cpu().numpy()[few, count[few] - 1]
    U.assert_close_fp32(only_at_count, s32[few], s64[few], RTOL, ATOL, "only at j = count")
    np.testing.assert_allclose(only_at_count, f.score.cpu().numpy()[few], rtol=2 * RTOL, atol=2 * ATOL)
    assert f.reached_only.cpu().numpy()[few, count[few] - 1].all()


def test_base_model_fidelity_walks_the_split():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    from tests.test_rules_gpu import _opt
    loader = DataLoader(ids=U.load("family_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 64), loader)
    out = bm.fidelity("test", k=2, batch=16, max_queries=40)
    assert out["n"] == 40 and out["k"] == 2
    for key in ("necessity_mean", "necessity_median", "sufficiency_gap_mean", "sufficiency_gap_median", "disconnected"):
        assert len(out[key]) == 2 and all(np.isfinite(v) for v in out[key]), key
    assert all(0.0 <= v <= 1.0 for v in out["disconnected"]) and out["disconnected"][0] <= out["disconnected"][1]
    one = bm.fidelity("test", k=2, batch=40, max_queries=40)                   # rows are independent of the batching
    assert one["disconnected"] == out["disconnected"]
    np.testing.assert_allclose(one["necessity_mean"], out["necessity_mean"], rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        bm.fidelity("train")


def test_temporal_digraph_is_refused():
    from red_gnn_amd.explain import RDigraph
    ids = _ids()
    loader = _loader(ids)
    model = _model(loader, 2, 16, 3, "idd")
    rd = model.explain(np.array([1, 2]), np.array([0, 1]))
    E = rd.edges.shape[0]
    t = RDigraph(**{**rd.__dict__, "time": torch.zeros(E, dtype=torch.int32, device="cuda"),
                    "q_time": torch.zeros(2, dtype=torch.int32, device="cuda")})
    with pytest.raises(ValueError, match="temporal"):
        t.rescore(model)
    with pytest.raises(ValueError, match="temporal"):
        t.fact_mask([(1, 0, 2)])
    with pytest.raises(ValueError, match="temporal"):
        t.top_paths(1).fact_mask(1)
