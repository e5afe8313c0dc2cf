"""RDigraph.integrated_gradients, model.integrated_gradients and the ``gate=`` of rescore / saliency on the MI355X (-m gpu), end to
end: against tests/ig_ref.py (saliency_ref's forward under the midpoint rule, fp64) at the same number of steps on the four cases of
tests/rescore_ref.py, with every edge kept and with the case's deletion mask, and on the inductive fixture.  Tolerance: the project's
stated one through tests/_util.assert_close_fp32, rtol 1e-4 and atol 2e-5 of the fp64 reference, or 4x the fp32 reference's own error;
compared are edge_attr, score, baseline_score and residual.  The residual is quadrature error and has no bound of its own here.
As measured on an MI355X, the worst |got - ref64| over every case: 6.4e-8 for edge_attr, 1.8e-7 for score, 9.2e-8 for baseline_score,
2.4e-7 for residual, at most 3.3 x the fp32 reference's own error on the same tensor and a hundredth of atol (information only).
Wall time of this file there: 7.0 s (15 tests)."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import ig_ref as IG
from tests import rescore_ref as R
from tests.test_explain_gpu import P
from tests.test_saliency_gpu import _setup

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
FIELDS = ("edge_attr", "score", "baseline_score", "residual")


def _compare(tag, att, ref64, ref32, e):
    assert np.array_equal(att.reached.cpu().numpy(), ref64["reached"]) and np.array_equal(att.live.cpu().numpy(), ref64["live"]), tag
    for name in FIELDS:
        got = getattr(att, name).cpu().numpy()
        print("%s %s: max |got - ref64| %.3g (ref32: %.3g; largest |value| %.3g)"
              % (tag, name, np.abs(got - ref64[name]).max(), np.abs(ref32[name] - ref64[name]).max(), np.abs(ref64[name]).max()))
        U.assert_close_fp32(got, ref32[name], ref64[name], RTOL, ATOL, "%s %s" % (tag, name))
    live, reached = ref64["live"], ref64["reached"]
    got = att.edge_attr.cpu().numpy()
    assert att.edge_attr.dtype == torch.float32 and att.edge_attr.shape == (len(e),) and att.digraph is not None
    # exactly 0: dead edges, rows that are not reached, and where target == baseline (the self-loops of the default baseline)
    assert (got[~live] == 0).all() and (got[~reached[e[:, 0]]] == 0).all(), tag
    for name in ("score", "baseline_score", "residual"):
        assert (getattr(att, name).cpu().numpy()[~reached] == 0).all(), "%s: %s of a row that is not reached" % (tag, name)


@pytest.mark.parametrize("name", list(R.CASES))
def test_integrated_gradients_against_the_reference(name):
    c, model, rd, e = _setup(name)
    ref = lambda steps, dt, **kw: IG.integrated_gradients(c.params, e, c.subs, c.rels, c.n_ent, c.n_rel, c.L, c.act, steps, dtype=dt, **kw)
    loops = e[:, 3] == 2 * c.n_rel
    att = {}
    for steps in (4, 16):
        att[steps] = rd.integrated_gradients(model, steps=steps)
        assert att[steps].steps == steps
        _compare("%s steps=%d" % (name, steps), att[steps], ref(steps, torch.float64), ref(steps, torch.float32), e)
        assert not att[steps].edge_attr[torch.as_tensor(loops).cuda()].any(), name + ": a self-loop of the default baseline has an attribution"
    assert torch.equal(att[4].score, att[16].score) and torch.equal(att[4].baseline_score, att[16].baseline_score)
    # ---- two identical calls: the same bits
    again = rd.integrated_gradients(model, steps=16)
    for field in FIELDS:
        assert torch.equal(getattr(again, field), getattr(att[16], field)), "%s: two calls differ in %s" % (name, field)
    # ---- the replicas in groups of 3 (6 launches per hop instead of 1): the dense products see other row counts, nothing else changes
    chunked = rd.integrated_gradients(model, steps=16, rep_chunk=3)
    _compare(name + " rep_chunk=3", chunked, ref(16, torch.float64), ref(16, torch.float32), e)
    np.testing.assert_allclose(chunked.edge_attr.cpu().numpy(), att[16].edge_attr.cpu().numpy(), rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(chunked.residual.cpu().numpy(), att[16].residual.cpu().numpy(), rtol=RTOL, atol=ATOL)
    # ---- a baseline and a target of the caller's own, as a tensor and as an array
    rng = np.random.default_rng(3)
    lo, hi = rng.uniform(0.0, 0.5, len(e)).astype(np.float32), rng.uniform(0.5, 1.25, len(e)).astype(np.float32)
    hi[::5] = lo[::5]                                                         # target == baseline: exactly 0
    own = rd.integrated_gradients(model, steps=4, baseline=torch.as_tensor(lo).cuda(), target=hi)
    _compare(name + " own path", own, ref(4, torch.float64, baseline=lo, target=hi), ref(4, torch.float32, baseline=lo, target=hi), e)
    assert not own.edge_attr[::5].any() and own.edge_attr.any()


@pytest.mark.parametrize("name", list(R.CASES))
def test_gates_of_one_are_the_ungated_calls_and_any_gate_matches_the_reference(name):
    c, model, rd, e = _setup(name)
    ones = torch.ones(len(e), device="cuda")
    for keep in (None, ~rd.fact_mask(c.facts, rows=c.fact_rows)):
        a, b = rd.rescore(model, keep=keep), rd.rescore(model, keep=keep, gate=ones)
        for field in ("score", "reached", "live", "alpha"):
            assert torch.equal(getattr(a, field), getattr(b, field)), "%s: rescore(gate=ones).%s" % (name, field)
        a, b = rd.saliency(model, keep=keep), rd.saliency(model, keep=keep, gate=np.ones(len(e), np.float32))
        for field in ("score", "reached", "live", "alpha", "edge_grad"):
            assert torch.equal(getattr(a, field), getattr(b, field)), "%s: saliency(gate=ones).%s" % (name, field)
    # ---- the gradient at a gate that is not 1, a 0 among its entries: live and reached stay structural
    g = np.random.default_rng(11).uniform(0.1, 1.4, len(e)).astype(np.float32)
    g[::7] = 0
    args = (c.params, e, c.subs, c.rels, c.n_ent, c.L, c.act, g)
    r64, r32 = IG.gradient_at(*args), IG.gradient_at(*args, dtype=torch.float32)
    sal, rs = rd.saliency(model, gate=torch.as_tensor(g).cuda()), rd.rescore(model, gate=g)
    assert bool(sal.live.all()) and bool(sal.reached.all()) and torch.equal(sal.score, rs.score) and torch.equal(sal.alpha, rs.alpha)
    print("%s: max |edge_grad - ref64| %.3g (ref32: %.3g), max |score - ref64| %.3g" % (name, np.abs(sal.edge_grad.cpu().numpy() - r64[4]).max(),
                                                                                         np.abs(r32[4] - r64[4]).max(), np.abs(sal.score.cpu().numpy() - r64[0]).max()))
    U.assert_close_fp32(sal.edge_grad.cpu().numpy(), r32[4], r64[4], RTOL, ATOL, name + " edge_grad at g")
    U.assert_close_fp32(sal.score.cpu().numpy(), r32[0], r64[0], RTOL, ATOL, name + " score at g")
    U.assert_close_fp32(sal.alpha.cpu().numpy(), r32[3], r64[3], RTOL, ATOL, name + " alpha at g")
    at_one = rd.saliency(model).edge_grad
    assert float((sal.edge_grad - at_one).abs().max()) > 1e-3 * float(at_one.abs().max())


@pytest.mark.parametrize("name", list(R.CASES))
def test_deleted_facts_leave_unreached_rows_at_exactly_zero(name):
    c, model, rd, e = _setup(name)
    keep = ~rd.fact_mask(c.facts, rows=c.fact_rows)
    k_h = keep.cpu().numpy()
    ref = lambda dt: IG.integrated_gradients(c.params, e, c.subs, c.rels, c.n_ent, c.n_rel, c.L, c.act, 4, keep=k_h, dtype=dt)
    r64 = ref(torch.float64)
    reached = r64["reached"]
    assert 4 * reached.sum() >= c.B and (~reached).any(), "the case must leave a quarter of the rows reached and cut one off"
    att = rd.integrated_gradients(model, steps=4, keep=keep)
    _compare(name + " facts deleted", att, r64, ref(torch.float32), e)
    gone = torch.as_tensor(~reached).cuda()
    assert not att.edge_attr[gone[rd.edges[:, 0].long()]].any() and not att.residual[gone].any() and not att.score[gone].any() \
        and not att.baseline_score[gone].any()
    assert torch.equal(rd.integrated_gradients(model, steps=4, keep=k_h.astype(np.uint8)).edge_attr, att.edge_attr)      # a host array goes along
    row, fact, attr = att.fact_attr()
    assert fact.shape[1] == 3 and len(att.format(k=2)) == c.B and att.top(2)[0].shape == (c.B, 2, 3)
    # with the default baseline the self-loops carry nothing, so a row's facts add up to the row's edges
    sums = torch.zeros(c.B, device="cuda").index_add(0, row, attr)
    np.testing.assert_allclose(sums.cpu().numpy(), (att.score - att.baseline_score - att.residual).cpu().numpy(), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("mode", ["transductive", "inductive"])
def test_integrated_gradients_inductive(mode):
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
    ref = lambda dt: IG.integrated_gradients(p, e, subs, rels, n_ent, loader.n_rel, n_layer, act, 4, dtype=dt)
    att = rd.integrated_gradients(model, steps=4, mode=mode)
    _compare(mode, att, ref(torch.float64), ref(torch.float32), e)
    by_model = model.integrated_gradients(subs, rels, steps=4, mode=mode)
    assert torch.equal(by_model.edge_attr, att.edge_attr) and torch.equal(by_model.digraph.edges, rd.edges)


def test_model_integrated_gradients_is_explain_then_the_digraph_call():
    c, model, rd, e = _setup("e300_L2")
    a, b = model.integrated_gradients(c.subs, c.rels, c.objs, steps=4), model.explain(c.subs, c.rels, c.objs).integrated_gradients(model, steps=4)
    for name in FIELDS + ("reached", "live"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.steps == 4 and torch.equal(a.digraph.edges, rd.edges)
    for p in model.parameters():
        assert p.grad is None                                 # the parameters are constants of the attribution
