"""Integrated gradients without a GPU: the reference of tests/ig_ref.py on its own - its gradient at a gate that is not 1 against
central differences, its quadrature error falling with the steps on the four cases of tests/rescore_ref.py - then
Attribution.fact_attr / top / format on a hand-made CPU digraph, and every refusal of RDigraph.integrated_gradients and of
``gate=`` that has to come before anything touches a device.

The reference's max |residual| in fp64, default baseline, as measured (steps 16 / 64): e300_L2 2.5e-4 / 1.5e-5, e300_L3 1.6e-3 /
1.2e-4, e60_L2 3.7e-3 / 1.3e-3, e60_L3 1.9e-3 / 1.2e-3 - the relu cases converge slowly (a kink inside a step).  It is quadrature
error, not rounding; the ordering is asserted, not these values."""
import inspect

import numpy as np
import pytest
import torch

from tests import ig_ref as IG
from tests import rescore_ref as R
from tests.test_fidelity_host import EDGES, _cpu_model, _digraph
from tests.test_tfidelity_host import _cpu_tmodel, _tdigraph
from tests.test_xfidelity_host import _cpu_xmodel, _xdigraph

_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = R.make_case(name, **R.CASES[name])
    return _CASES[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_gradient_at_a_random_gate_matches_central_differences(name):
    c = _case(name)
    gate = np.random.default_rng(5).uniform(0.1, 1.4, len(c.edges))
    args = (c.params, c.edges, c.subs, c.rels, c.n_ent, c.L, c.act)
    score, reached, live, alpha, grad = IG.gradient_at(*args, gate)
    fd = IG.finite_differences_at(*args, gate, None, live)
    scale = np.abs(grad).max()
    print("%s: max |autograd - central differences| %.3g, largest |gradient| %.3g" % (name, np.abs(grad - fd).max(), scale))
    assert scale > 0 and live.all() and reached.all()
    # a central difference with step h = 1e-6 in fp64 carries rounding of about 2^-53 |score| / h ~ 1e-10 and truncation of h^2 f''' / 6
    # ~ 1e-13: the bound is a hundred times the first.  (relu: a pre-activation within h of 0 would make the quotient one-sided; none
    # of the cases has one at this gate)
    np.testing.assert_allclose(grad, fd, rtol=1e-5, atol=1e-7 * scale)
    at_one = IG.gradient_at(*args, np.ones(len(c.edges)))[4]
    assert np.abs(grad - at_one).max() > 1e-3 * scale                       # the gate matters: this is not the gradient at 1


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_residual_falls_with_the_steps(name):
    c = _case(name)
    args = (c.params, c.edges, c.subs, c.rels, c.n_ent, c.n_rel, c.L, c.act)
    r16, r64 = IG.integrated_gradients(*args, 16), IG.integrated_gradients(*args, 64)
    worst = [np.abs(r["residual"]).max() for r in (r16, r64)]
    print("%s: max |residual| %.3g at 16 steps, %.3g at 64" % (name, *worst))
    assert worst[1] < worst[0]
    assert np.array_equal(r16["score"], r64["score"]) and np.array_equal(r16["baseline_score"], r64["baseline_score"])
    loops = np.asarray(c.edges)[:, 3] == 2 * c.n_rel
    assert (r16["edge_attr"][loops] == 0).all() and np.abs(r16["edge_attr"][~loops]).max() > 0      # hi == lo on the self-loops
    f32 = IG.integrated_gradients(*args, 16, dtype=torch.float32)
    assert np.abs(f32["edge_attr"] - r16["edge_attr"]).max() < 1e-6          # rounding is not what the residual is made of


# ---- Attribution on a hand-made digraph (tests/test_fidelity_host.EDGES; powers of two: every sum is exact) -------------------------
ATTR = [0.0, 2.0, 0.0, 8.0, 0.0, 32.0, 0.0, 128.0, -512.0]


def _attribution(attr=ATTR):
    from red_gnn_amd.explain import Attribution
    return Attribution(score=torch.tensor([1.0, 2.0]), baseline_score=torch.tensor([0.5, 0.25]), edge_attr=torch.tensor(attr),
                       residual=torch.zeros(2), reached=torch.tensor([True, True]), live=torch.ones(9, dtype=torch.bool), steps=4,
                       digraph=_digraph(EDGES, 2))


def test_attribution_groups_like_saliency():
    from red_gnn_amd.explain import Saliency
    a = _attribution()
    row, fact, attr = a.fact_attr()
    assert row.tolist() == [0, 1, 1] and fact.tolist() == [[5, 0, 6], [5, 0, 6], [5, 1, 6]] and attr.tolist() == [10.0, 160.0, -512.0]
    assert row.dtype == fact.dtype == torch.int64 and attr.dtype == torch.float32
    s = Saliency(score=a.score, reached=a.reached, live=a.live, alpha=torch.full((9,), 0.5), edge_grad=a.edge_attr, digraph=a.digraph)
    assert all(torch.equal(x, y) for x, y in zip(a.fact_attr(), s.fact_grad()))       # one grouping, shared
    assert all(torch.equal(x, y) for x, y in zip(a.top(2), s.top(2)))
    fact, attr, count = a.top(1)
    assert fact.tolist() == [[[5, 0, 6]], [[5, 1, 6]]] and attr.tolist() == [[10.0], [-512.0]] and count.tolist() == [1, 1]
    a.reached = torch.tensor([True, False])
    assert a.format() == ["row 0: score 1.0000  (5, r0, 6) +10.0000", "row 1: score x  (5, r1, 6) -512.0000  (5, r0, 6) +160.0000"]
    assert a.format(id2rel=["a", "b", "c"], k=1)[1] == "row 1: score x  (5, b, 6) -512.0000"
    with pytest.raises(ValueError, match="fact_attr: inverse_offset"):
        a.fact_attr(inverse_offset=3)
    with pytest.raises(ValueError, match="top: k"):
        a.top(0)


# ---- the refusals: all ValueError, all before any HIP call ---------------------------------------------------------------------------
def test_timed_digraphs_and_models_are_refused():
    static, tmodel, xmodel = _cpu_model(), _cpu_tmodel(), _cpu_xmodel()
    st, td, xd = _digraph(EDGES, 2), _tdigraph(), _xdigraph()
    ones = lambda rd: torch.ones(rd.edges.shape[0])
    for rd, model in ((td, static), (xd, static), (td, tmodel), (xd, xmodel), (st, tmodel), (st, xmodel)):
        with pytest.raises(ValueError, match="integrated_gradients: .*timed forms are not built"):
            rd.integrated_gradients(model)
        with pytest.raises(ValueError, match="rescore: .*timed forms are not built"):
            rd.rescore(model, gate=ones(rd))
        with pytest.raises(ValueError, match="saliency: .*timed forms are not built"):
            rd.saliency(model, gate=ones(rd))


def test_steps_gates_baselines_and_targets_are_checked_on_the_host():
    model, rd = _cpu_model(), _digraph(EDGES, 2)
    for steps in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="integrated_gradients: steps"):
            rd.integrated_gradients(model, steps=steps)
    with pytest.raises(ValueError, match="integrated_gradients: rep_chunk"):
        rd.integrated_gradients(model, rep_chunk=0)
    nan, inf = torch.ones(9), torch.ones(9)
    nan[3], inf[8] = float("nan"), float("-inf")
    bad = ((torch.ones(8), "float32 \\[9\\]"), (torch.ones(9, dtype=torch.float64), "float32 \\[9\\]"), (np.ones(9), "float32 \\[9\\]"),
           (torch.ones(9, dtype=torch.bool), "float32 \\[9\\]"), (torch.ones((9, 1)), "float32 \\[9\\]"), (nan, "not finite"), (inf, "not finite"),
           (np.full(9, np.inf, np.float32), "not finite"))
    for g, text in bad:
        with pytest.raises(ValueError, match="rescore: gate .*" + text):
            rd.rescore(model, gate=g)
        with pytest.raises(ValueError, match="saliency: gate .*" + text):
            rd.saliency(model, gate=g)
        with pytest.raises(ValueError, match="integrated_gradients: baseline .*" + text):
            rd.integrated_gradients(model, baseline=g)
        with pytest.raises(ValueError, match="integrated_gradients: target .*" + text):
            rd.integrated_gradients(model, target=g)
    # the digraph's and keep's own checks keep their words, under the caller's name
    with pytest.raises(ValueError, match="integrated_gradients: keep must be bool"):
        rd.integrated_gradients(model, keep=torch.ones(9))
    with pytest.raises(ValueError, match="integrated_gradients: .*n_hops=3"):
        _digraph(EDGES, 2, n_hops=3).integrated_gradients(model)
    # all in order: then the device is asked for
    for kw in (dict(), dict(baseline=np.zeros(9, np.float32), target=torch.ones(9), steps=3, rep_chunk=2)):
        with pytest.raises(ValueError, match="integrated_gradients: .*on one device"):
            rd.integrated_gradients(model, **kw)
    with pytest.raises(ValueError, match="rescore: .*on one device"):
        rd.rescore(model, gate=torch.ones(9))


def test_signatures_and_bindings():
    from red_gnn_amd import _lib, engine, explain
    from red_gnn_amd.models import RED_GNN_induc, RED_GNN_trans
    sig = inspect.signature(explain.RDigraph.integrated_gradients).parameters
    assert list(sig)[1:] == ["model", "steps", "keep", "baseline", "target", "rep_chunk", "mode"] and sig["steps"].default == 16
    for f in (explain.RDigraph.rescore, explain.RDigraph.saliency):
        assert list(inspect.signature(f).parameters)[1:] == ["model", "keep", "mode", "gate"]
    assert list(inspect.signature(RED_GNN_trans.integrated_gradients).parameters)[1:] == ["subs", "rels", "objs", "steps", "mode"]
    assert inspect.signature(RED_GNN_induc.integrated_gradients).parameters["mode"].default == "transductive"
    L = _lib.lib()
    assert len(L.rg_digraph_layer_fwd_gated.argtypes) == 30 and len(L.rg_digraph_layer_bwd_gated.argtypes) == 33
    assert callable(engine.digraph_layer_fwd_gated) and callable(engine.digraph_layer_bwd_gated)
    # scratch: the chunk list once, the partial rows once per replica
    ptr = np.array([0, 5, 305, 306, 1000], np.int32)
    fwd = lambda n: L.rg_digraph_layer_fwd_gated_scratch_bytes(_lib.ptr(ptr), 4, 20, n)
    bwd = lambda n: L.rg_digraph_layer_bwd_gated_scratch_bytes(_lib.ptr(ptr), 4, 20, 32, n)
    up = lambda b: (b + 255) // 256 * 256
    assert fwd(1) == L.rg_digraph_layer_fwd_scratch_bytes(_lib.ptr(ptr), 4, 20) and bwd(1) == L.rg_digraph_layer_bwd_scratch_bytes(_lib.ptr(ptr), 4, 20, 32)
    assert fwd(5) == 256 + up(5 * 9 * 20 * 4) and bwd(5) == 256 + up(5 * 9 * 20 * 4) + up(5 * 9 * 32 * 4) and fwd(0) == 0 and bwd(0) == 0
