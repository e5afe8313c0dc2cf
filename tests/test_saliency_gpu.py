"""RDigraph.saliency and model.saliency on the MI355X (-m gpu), end to end: against tests/saliency_ref.py (rescore_ref's forward in torch
with a gate on every edge's message, the gradient by autograd) on the four cases of tests/rescore_ref.py, with every edge kept and with
the case's deletion mask, and against RDigraph.rescore on the same digraph.  Tolerance: the project's stated one through
tests/_util.assert_close_fp32, rtol 1e-4 and atol 2e-5 of the fp64 reference, or 4x the fp32 reference's own error."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import rescore_ref as R
from tests import saliency_ref as S
from tests.test_explain_gpu import P, _loader, _model

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
_CACHE = {}


def _setup(name):
    """The case, its model (rescore_ref.random_params loaded into a RED_GNN_trans over the case's triples) and its digraph."""
    if name not in _CACHE:
        c = R.make_case(name, **R.CASES[name])
        ids = dict(n_ent=c.n_ent, n_rel=c.n_rel, facts=c.triples[:-1], train=c.triples[-1:], valid=c.triples[:1], test=c.triples[:1])
        loader = _loader(ids)                                   # the evaluation graph: facts + train = the case's triples, in order
        model = _model(loader, c.L, c.d, c.attn, c.act)
        model.load_state_dict({k: torch.tensor(v) for k, v in c.params.items()}, strict=True)
        rd = model.explain(c.subs, c.rels, c.objs)
        e = rd.edges.cpu().numpy().astype(np.int64)
        assert np.array_equal(U.sorted_edges(e), U.sorted_edges(c.edges)) and bool(rd.reached.all())
        _CACHE[name] = (c, model, rd, e)
    return _CACHE[name]


def _compare(tag, sal, rs, ref64, ref32, e):
    score, reached, live, alpha, grad = ref64
    assert np.array_equal(sal.reached.cpu().numpy(), reached) and np.array_equal(sal.live.cpu().numpy(), live), tag + ": reached / live"
    assert torch.equal(sal.reached, rs.reached) and torch.equal(sal.live, rs.live), tag + ": reached / live against rescore"
    assert torch.equal(sal.alpha, rs.alpha), tag + ": alpha is rescore's, bit for bit"
    got_s, got_g = sal.score.cpu().numpy(), sal.edge_grad.cpu().numpy()
    scale = np.abs(grad).max()
    print("%s: max |edge_grad - ref64| %.3g (ref32: %.3g; largest |gradient| %.3g), max |score - ref64| %.3g (ref32: %.3g)"
          % (tag, np.abs(got_g - grad).max(), np.abs(ref32[4] - grad).max(), scale, np.abs(got_s - score).max(), np.abs(ref32[0] - score).max()))
    U.assert_close_fp32(got_g, ref32[4], grad, RTOL, ATOL, tag + " edge_grad")
    U.assert_close_fp32(got_s, ref32[0], score, RTOL, ATOL, tag + " score")
    np.testing.assert_allclose(got_s, rs.score.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)
    assert sal.edge_grad.dtype == torch.float32 and sal.edge_grad.shape == (len(e),) and sal.digraph is not None
    # exactly 0: dead edges, rows that are not reached
    assert (got_g[~live] == 0).all() and (got_g[~reached[e[:, 0]]] == 0).all() and (got_s[~reached] == 0).all(), tag
    assert np.abs(got_g[live & reached[e[:, 0]]]).max() > 0


@pytest.mark.parametrize("name", list(R.CASES))
def test_saliency_against_the_reference_and_rescore(name):
    c, model, rd, e = _setup(name)
    ref = lambda keep, dt: S.saliency(c.params, e, c.subs, c.rels, c.n_ent, c.L, c.act, keep=keep, dtype=dt)

    # ---- every edge kept
    sal = rd.saliency(model)
    _compare(name + " keep=None", sal, rd.rescore(model), ref(None, torch.float64), ref(None, torch.float32), e)
    assert bool(sal.live.all()) and bool(sal.reached.all())
    again = rd.saliency(model)
    assert torch.equal(again.edge_grad, sal.edge_grad) and torch.equal(again.score, sal.score), name + ": two calls differ"

    # ---- the case's facts deleted, each for its own row
    m = rd.fact_mask(c.facts, rows=c.fact_rows)
    assert np.array_equal(m.cpu().numpy(), R.fact_mask(e, c.n_rel, c.facts, c.fact_rows))
    keep = ~m
    k_h = keep.cpu().numpy()
    cut = rd.saliency(model, keep=keep)
    r64 = ref(k_h, torch.float64)
    reached = r64[1]
    print("%s: %d of %d edges kept, %d live, %d of %d rows reached" % (name, k_h.sum(), len(e), r64[2].sum(), reached.sum(), c.B))
    assert 4 * reached.sum() >= c.B and (~reached).any(), "the case must leave a quarter of the rows reached and cut one off"
    _compare(name + " facts deleted", cut, rd.rescore(model, keep=keep), r64, ref(k_h, torch.float32), e)
    gone = torch.as_tensor(~reached).cuda()[rd.edges[:, 0].long()]
    assert gone.any() and not cut.edge_grad[gone].any(), name + ": a disconnected row has a gradient"
    again = rd.saliency(model, keep=k_h.astype(np.uint8))                             # a host array goes along, bits unchanged
    assert torch.equal(again.edge_grad, cut.edge_grad) and torch.equal(again.score, cut.score)
    # the first-order estimate is finite and leaves disconnected rows at 0
    est = sal.deletion_estimate(m)
    assert est.shape == (c.B,) and bool(torch.isfinite(est).all())
    assert len(sal.format()) == c.B and sal.top(2)[0].shape == (c.B, 2, 3)


@pytest.mark.parametrize("mode", ["transductive", "inductive"])
def test_saliency_inductive(mode):
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    fx, ids = U.load("ind_WN18RR_v1_%s.npz" % mode), U.load("ind_WN18RR_v1_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    act = str(fx["act"])
    model = RED_GNN_induc(P(n_layer, d, a, loader.n_rel, act), loader).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    subs, rels = fx["subs"].astype(np.int64)[:12], fx["rels"].astype(np.int64)[:12]
    n_ent = loader.graph_for(mode).n_ent
    rd = model.explain(subs, rels, mode=mode)                 # each row's own top answer
    e = rd.edges.cpu().numpy().astype(np.int64)
    p = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    ref = lambda dt: S.saliency(p, e, subs, rels, n_ent, n_layer, act, dtype=dt)
    sal = rd.saliency(model, mode=mode)
    _compare(mode, sal, rd.rescore(model, mode=mode), ref(torch.float64), ref(torch.float32), e)
    by_model = model.saliency(subs, rels, mode=mode)
    assert torch.equal(by_model.edge_grad, sal.edge_grad) and torch.equal(by_model.digraph.edges, rd.edges)


def test_model_saliency_is_explain_then_saliency():
    c, model, rd, e = _setup("e300_L2")
    a, b = model.saliency(c.subs, c.rels, c.objs), model.explain(c.subs, c.rels, c.objs).saliency(model)
    for name in ("score", "reached", "live", "alpha", "edge_grad"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.digraph.edges, rd.edges)
    for p in model.parameters():
        assert p.grad is None                                 # the parameters are constants of the saliency


def test_temporal_digraph_is_refused():
    from red_gnn_amd.explain import RDigraph
    c, model, rd, e = _setup("e300_L2")
    t = RDigraph(**{**rd.__dict__, "time": torch.zeros(len(e), dtype=torch.int32, device="cuda"),
                    "q_time": torch.zeros(c.B, dtype=torch.int32, device="cuda")})
    with pytest.raises(ValueError, match="temporal"):
        t.saliency(model)
