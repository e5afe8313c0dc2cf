"""RDigraph.saliency and model.saliency of the two temporal models on the MI355X (-m gpu), end to end: against tests/tsaliency_ref.py
(the rescore references' forward in torch with a gate on every edge's message, the gradient by autograd) on the cases of
tests/test_trescore_gpu.py (temporal_ref.hand_graph) and tests/test_xrescore_gpu.py (extrap_ref.make_case), with every edge kept and
with the case's deletion mask, and against RDigraph.rescore on the same digraph.  Tolerance: the project's stated one through
tests/_util.assert_close_fp32, rtol 1e-4 and atol 2e-5 of the fp64 reference, or 4x the fp32 reference's own error."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import extrap_ref as XR
from tests import temporal_ref as TR
from tests import trescore_ref as TRS
from tests import tsaliency_ref as S
from tests import xrescore_ref as XRS
from tests.test_trescore_gpu import CONFIGS as T_CONFIGS, M, N_ENT as T_N_ENT, _model as _t_model
from tests.test_xrescore_gpu import CASES as X_CASES, _setup as _x_setup

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5


def _compare(tag, sal, rs, ref64, ref32, e):
    score, reached, live, alpha, grad = ref64
    assert np.array_equal(sal.reached.cpu().numpy(), reached) and np.array_equal(sal.live.cpu().numpy(), live), tag + ": reached / live"
    # score, reached, live and alpha are rescore's, bit for bit
    for name in ("score", "reached", "live", "alpha"):
        assert torch.equal(getattr(sal, name), getattr(rs, name)), "%s: %s is not rescore's" % (tag, name)
    got_s, got_g = sal.score.cpu().numpy(), sal.edge_grad.cpu().numpy()
    print("%s: max |edge_grad - ref64| %.3g (ref32: %.3g; largest |gradient| %.3g), max |score - ref64| %.3g (ref32: %.3g)"
          % (tag, np.abs(got_g - grad).max(), np.abs(ref32[4] - grad).max(), np.abs(grad).max(), np.abs(got_s - score).max(),
             np.abs(ref32[0] - score).max()))
    U.assert_close_fp32(got_g, ref32[4], grad, RTOL, ATOL, tag + " edge_grad")
    U.assert_close_fp32(got_s, ref32[0], score, RTOL, ATOL, tag + " score")
    assert sal.edge_grad.dtype == torch.float32 and sal.edge_grad.shape == (len(e),) and sal.digraph is not None
    # exactly 0: dead edges, rows that are not reached
    assert (got_g[~live] == 0).all() and (got_g[~reached[e[:, 0]]] == 0).all() and (got_s[~reached] == 0).all(), tag
    assert np.abs(got_g[live & reached[e[:, 0]]]).max() > 0


def _both_ways(tag, model, rd, e, ref, mask, before):
    """Every edge kept, then the deletion ``mask``: against the reference and rescore, two calls bit for bit, no parameter gradient."""
    sal = rd.saliency(model)
    _compare(tag + " keep=None", sal, rd.rescore(model), ref(None, torch.float64), ref(None, torch.float32), e)
    assert bool(sal.live.all())
    again = rd.saliency(model)
    assert torch.equal(again.edge_grad, sal.edge_grad) and torch.equal(again.score, sal.score), tag + ": two calls differ"
    keep = ~mask
    k_h = keep.cpu().numpy()
    r64 = ref(k_h, torch.float64)
    reached = r64[1]
    print("%s: %d of %d edges kept, %d live, %d of %d rows reached" % (tag, k_h.sum(), len(e), r64[2].sum(), reached.sum(), len(reached)))
    # the condition of the deletion mask, with the reference alone
    assert 4 * reached.sum() >= len(reached) and (before & ~reached).any(), "the mask must leave a quarter of the rows reached and cut one off"
    cut = rd.saliency(model, keep=keep)
    _compare(tag + " facts deleted", cut, rd.rescore(model, keep=keep), r64, ref(k_h, torch.float32), e)
    gone = torch.as_tensor(~reached).cuda()[rd.edges[:, 0].long()]
    assert gone.any() and not cut.edge_grad[gone].any(), tag + ": a disconnected row has a gradient"
    again = rd.saliency(model, keep=k_h.astype(np.uint8))                             # a host array goes along, bits unchanged
    assert torch.equal(again.edge_grad, cut.edge_grad) and torch.equal(again.score, cut.score)
    for p in model.parameters():
        assert p.grad is None                                                         # the parameters are constants of the saliency
    est = sal.deletion_estimate(mask)
    assert est.shape == (len(reached),) and bool(torch.isfinite(est).all())
    assert len(sal.format()) == len(reached) and sal.top(2)[0].shape == (len(reached), 2, 4)
    return sal


@pytest.mark.parametrize("d,a,act,L,shared", T_CONFIGS)
def test_temporal_saliency_against_the_reference_and_rescore(d, a, act, L, shared):
    quads, heads, rels, times, objs, deleted = TRS.inputs(L)
    model = _t_model(quads, d, a, act, L, shared)
    batch = {"head": heads, "relation": rels, "time": times}
    rd = model.explain(batch, objs)
    e, t = rd.edges.cpu().numpy().astype(np.int64), rd.time.cpu().numpy().astype(np.int64)
    p = TR.state_of(model)
    ref = lambda keep, dt: S.saliency("temporal", p, e, t, times, heads, rels, T_N_ENT, L, act, keep=keep, shared_tables=shared, dtype=dt)
    tag = "temporal d%d a%d %s L%d shared=%s" % (d, a, act, L, shared)
    sal = _both_ways(tag, model, rd, e, ref, rd.fact_mask(deleted, inverse_offset=M), np.ones(len(heads), bool))
    # model.saliency is explain, then saliency
    by_model = model.saliency(batch, objs)
    for name in ("score", "reached", "live", "alpha", "edge_grad"):
        assert torch.equal(getattr(by_model, name), getattr(sal, name)), name
    assert torch.equal(by_model.digraph.edges, rd.edges) and torch.equal(by_model.digraph.time, rd.time)
    # a fact's gradient is the sum over the edges its mask marks, in its row
    row, fact, grad = sal.fact_grad(inverse_offset=M)
    assert fact.shape[1] == 4 and int(fact[:, 1].max()) < M and int(fact[:, 3].max()) < TR.HAND_N_TIME
    for i in np.random.default_rng(0).choice(len(row), 5, replace=False):
        m = rd.fact_mask(fact[i:i + 1], rows=row[i:i + 1], inverse_offset=M)
        np.testing.assert_allclose(float(grad[i]), float(sal.edge_grad[m].double().sum()), rtol=1e-5, atol=1e-6)
    was_training = model.training
    model.train()
    try:
        assert torch.equal(rd.saliency(model).edge_grad, sal.edge_grad) and model.training   # eval semantics, and the flag comes back
    finally:
        model.train(was_training)


@pytest.mark.parametrize("d,a,act,L,B", X_CASES)
def test_extrapolation_saliency_against_the_reference_and_rescore(d, a, act, L, B):
    model, data, rows, objs, q_day, rd = _x_setup(d, a, act, L, B)
    e, day, data_row = (x.cpu().numpy().astype(np.int64) for x in (rd.edges, rd.time, rd.data_row))
    p = TR.state_of(model)
    ref = lambda keep, dt: S.saliency("extrapolation", p, e, day, q_day, rows[:, 0], rows[:, 1], XR.N_ENT, L, act, keep=keep, dtype=dt)
    tag = "extrapolation d%d a%d %s L%d" % (d, a, act, L)
    facts = XRS.deleted_facts(data, e, data_row, day, rows[:, 0])
    sal = _both_ways(tag, model, rd, e, ref, rd.fact_mask(facts), rd.reached.cpu().numpy())
    by_model = model.saliency(XR.Batch(rows), objs)
    for name in ("score", "reached", "live", "alpha", "edge_grad"):
        assert torch.equal(getattr(by_model, name), getattr(sal, name)), name
    assert torch.equal(by_model.digraph.edges, rd.edges) and torch.equal(by_model.digraph.data_row, rd.data_row)
    # data rows: the exact identity of a fact
    row, dr, grad = sal.data_row_grad()
    assert int(dr.min()) >= 0 and row.shape == dr.shape == grad.shape
    for i in np.random.default_rng(0).choice(len(row), 5, replace=False):
        m = rd.data_row_mask(dr[i:i + 1], rows=row[i:i + 1])
        np.testing.assert_allclose(float(grad[i]), float(sal.edge_grad[m].double().sum()), rtol=1e-5, atol=1e-6 * max(1.0, float(grad[i].abs())))
    for frs in model._frontiers.pool.values():                                        # no frontier is left with a window set
        assert all(getattr(fr, "_window", None) is None for fr in frs)


def test_a_digraph_of_the_wrong_family_is_refused():
    quads, heads, rels, times, objs, _ = TRS.inputs(2)
    tmodel = _t_model(quads, 16, 3, "idd", 2, False)
    td = tmodel.explain({"head": heads, "relation": rels, "time": times}, objs)
    xmodel, data, rows, xobjs, q_day, xd = _x_setup(*XR.CASES[2])
    with pytest.raises(ValueError, match="saliency: a temporal.T_RED_GNN .*extrapolation r-digraph"):
        xd.saliency(tmodel)
    with pytest.raises(ValueError, match="saliency: an extrapolation.T_RED_GNN .*temporal interpolation r-digraph"):
        td.saliency(xmodel)
    static = type(td)(**{**td.__dict__, "time": None, "q_time": None, "n_time": None})
    with pytest.raises(ValueError, match="saliency: a temporal.T_RED_GNN .*static r-digraph"):
        static.saliency(tmodel)
    with pytest.raises(ValueError, match="saliency: .*mode must be 'test'"):
        td.saliency(tmodel, mode="valid")
    with pytest.raises(ValueError, match="saliency: .*n_layer=3"):
        td.saliency(_t_model(quads, 16, 3, "idd", 3, False))
    assert torch.equal(td.saliency(tmodel).reached, td.reached)                       # and the model still answers
