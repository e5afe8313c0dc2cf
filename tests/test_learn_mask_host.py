"""RDigraph.learn_mask without a GPU: every refusal that has to come before anything touches a device, in the order the arguments
are checked; EdgeMask.fact_gate / top / format / sufficiency_gap and the selection rule on hand-built tensors; the new symbols in
the header and in the binding."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.test_fidelity_host import EDGES, _cpu_model, _digraph
from tests.test_tfidelity_host import _cpu_tmodel, _tdigraph
from tests.test_xfidelity_host import _cpu_xmodel, _xdigraph


def test_arguments_are_checked_on_the_host_in_order():
    model, rd = _cpu_model(), _digraph(EDGES, 2)
    inf, nan = float("inf"), float("nan")
    for lambdas in ((), [], None, 0.1, (0.1, -0.2), (nan,), (0.1, inf), "ab", ((0.1, 0.2),)):
        with pytest.raises(ValueError, match="learn_mask: lambdas"):
            rd.learn_mask(model, lambdas=lambdas, iterations=-1)              # lambdas come first
    for entropy in (-0.1, nan, None, True):
        with pytest.raises(ValueError, match="learn_mask: entropy"):
            rd.learn_mask(model, entropy=entropy, iterations=-1)
    for iterations in (-1, 1.5, True, None, "3"):
        with pytest.raises(ValueError, match="learn_mask: iterations"):
            rd.learn_mask(model, iterations=iterations, lr=0)
    for lr in (0, -0.05, nan, inf, None):
        with pytest.raises(ValueError, match="learn_mask: lr"):
            rd.learn_mask(model, lr=lr, tol=-1)
    for tol in (-0.01, nan, None):
        with pytest.raises(ValueError, match="learn_mask: tol"):
            rd.learn_mask(model, tol=tol, theta0=nan)
    for theta0 in (nan, inf, -inf, None, "2"):
        with pytest.raises(ValueError, match="learn_mask: theta0"):
            rd.learn_mask(model, theta0=theta0)
    # its own arguments come before the timed refusal, the refusal before the digraph's tensors
    with pytest.raises(ValueError, match="learn_mask: theta0"):
        _tdigraph().learn_mask(model, theta0=nan)
    with pytest.raises(ValueError, match="learn_mask: .*timed forms are not built"):
        _tdigraph().learn_mask(model, keep=torch.ones(3))
    # the digraph's and keep's own checks keep their words, under the caller's name
    with pytest.raises(ValueError, match="learn_mask: alpha must be float32"):
        _digraph(EDGES, 2, alpha=torch.zeros(8)).learn_mask(model)
    with pytest.raises(ValueError, match="learn_mask: keep must be bool"):
        rd.learn_mask(model, keep=torch.ones(9))
    with pytest.raises(ValueError, match="learn_mask: .*n_hops=3"):
        _digraph(EDGES, 2, n_hops=3).learn_mask(model)
    # all in order (iterations = 0 and a lambda of 0 are allowed): then the device is asked for
    for kw in (dict(), dict(lambdas=[0.0], iterations=0, tol=0, entropy=0.1, theta0=-1, lr=1e-3), dict(lambdas=np.array([0.5, 0.25]))):
        with pytest.raises(ValueError, match="learn_mask: .*on one device"):
            rd.learn_mask(model, **kw)


def test_timed_digraphs_and_models_are_refused():
    static, tmodel, xmodel = _cpu_model(), _cpu_tmodel(), _cpu_xmodel()
    st, td, xd = _digraph(EDGES, 2), _tdigraph(), _xdigraph()
    for rd, model in ((td, static), (xd, static), (td, tmodel), (xd, xmodel), (st, tmodel), (st, xmodel)):
        with pytest.raises(ValueError, match="learn_mask: .*timed forms are not built"):
            rd.learn_mask(model)


GATE = [1.0, 0.25, 1.0, 0.75, 1.0, 0.5, 1.0, 0.125, 0.875]


def _mask(gate=GATE):
    from red_gnn_amd.explain import EdgeMask
    import types
    g = torch.tensor(gate)
    loops = torch.tensor(EDGES)[:, 3] == 6
    z = torch.zeros(2)
    return EdgeMask(gate=g, keep=(g > 0.5) | loops, score=torch.tensor([1.0, 2.0]), hard_score=z, kept_score=torch.tensor([0.75, 2.5]),
                    target=torch.tensor([1.0, 2.25]), baseline_score=z, size=torch.tensor([1, 1]), n_free=torch.tensor([2, 3]),
                    replica=torch.tensor([0, 1]), lambdas=torch.tensor([0.1, 0.3]), history=types.SimpleNamespace(),
                    reached=torch.tensor([True, True]), live=torch.ones(9, dtype=torch.bool), digraph=_digraph(EDGES, 2))


def test_edge_mask_groups_by_fact_and_takes_the_largest_gate():
    mk = _mask()
    row, fact, gate = mk.fact_gate()
    # row 0: (5, 0, 6) is edges 1 and 3, the larger gate; row 1: (5, 0, 6) is edges 5 and 7, (5, 1, 6) edge 8; the self-loops are no facts
    assert row.tolist() == [0, 1, 1] and fact.tolist() == [[5, 0, 6], [5, 0, 6], [5, 1, 6]] and gate.tolist() == [0.75, 0.5, 0.875]
    assert row.dtype == fact.dtype == torch.int64 and gate.dtype == torch.float32
    fact, gate, count = mk.top(1)
    assert fact.tolist() == [[[5, 0, 6]], [[5, 1, 6]]] and gate.tolist() == [[0.75], [0.875]] and count.tolist() == [1, 1]
    assert mk.top(3)[2].tolist() == [1, 2]
    mk.reached = torch.tensor([True, False])
    assert mk.format() == ["row 0: score 1.0000  (5, r0, 6) +0.7500", "row 1: score x  (5, r1, 6) +0.8750  (5, r0, 6) +0.5000"]
    assert mk.format(id2rel=["a", "b", "c"], k=1)[1] == "row 1: score x  (5, b, 6) +0.8750"
    assert mk.sufficiency_gap().tolist() == [0.25, -0.25]
    with pytest.raises(ValueError, match="top: k"):
        mk.top(0)
    # the sums of Saliency / Attribution are untouched by the other reduction
    from red_gnn_amd.explain import Saliency
    s = Saliency(score=mk.score, reached=mk.reached, live=mk.live, alpha=torch.full((9,), 0.5), edge_grad=mk.gate, digraph=mk.digraph)
    assert s.fact_grad()[2].tolist() == [1.0, 0.625, 0.875]


def test_selection_rule():
    from red_gnn_amd.explain import mask_selection
    target, scale = torch.tensor([1.0, 1.0, 1.0, 0.0, 1.0]), torch.tensor([2.0, 2.0, 2.0, 0.0, 2.0])
    #                      row 0: 1 and 2 qualify,    row 1: none: the       row 2: a tie in    row 3: scale 0,      row 4: all qualify,
    #                      2 is smaller               smallest deviation     size: the lower    all exact: smallest  equal sizes: replica 0
    hard = torch.tensor([[0.00, 0.00, 1.00, 0.0, 1.0],
                         [1.05, 0.50, 1.00, 0.0, 1.0],
                         [0.95, 0.50, 0.00, 0.0, 1.0]])
    size = torch.tensor([[1, 9, 4, 5, 3],
                         [7, 5, 4, 2, 3],
                         [3, 1, 0, 2, 3]])
    assert mask_selection(hard, size, target, scale, 0.05).tolist() == [2, 1, 0, 1, 0]
    assert mask_selection(hard, size, target, scale, 0.0).tolist() == [1, 1, 0, 1, 0]           # row 0: nothing within 0: the smallest deviation
    assert mask_selection(hard[:1], size[:1], target, scale, 0.05).tolist() == [0] * 5


def test_signatures_and_bindings():
    from red_gnn_amd import _lib, engine, explain
    from red_gnn_amd.models import RED_GNN_induc, RED_GNN_trans
    sig = inspect.signature(explain.RDigraph.learn_mask).parameters
    assert list(sig)[1:] == ["model", "lambdas", "entropy", "iterations", "lr", "theta0", "tol", "keep", "mode"]
    want = dict(lambdas=(0.01, 0.03, 0.1, 0.3, 1.0), entropy=0.0, iterations=100, lr=0.05, theta0=2.0, tol=0.05, keep=None, mode="test")
    assert {k: sig[k].default for k in want} == want
    assert list(inspect.signature(RED_GNN_trans.learn_mask).parameters)[1:4] == ["subs", "rels", "objs"]
    assert inspect.signature(RED_GNN_induc.learn_mask).parameters["mode"].default == "transductive"
    names = ("rg_digraph_layer_fwd_gates", "rg_digraph_layer_bwd_gates", "rg_mask_step")
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "redgnn.h")).read()
    for name in names:
        assert name in _lib.SYMBOLS and ("int %s(" % name) in header, name
    assert "#define RG_MASK_CHUNK %d" % engine.MASK_CHUNK in header
    L = _lib.lib()
    assert L.rg_version() == 12
    assert len(L.rg_digraph_layer_fwd_gates.argtypes) == 28 and len(L.rg_digraph_layer_bwd_gates.argtypes) == 31
    assert len(L.rg_mask_step.argtypes) == 24
    for f in (engine.digraph_layer_fwd_gates, engine.digraph_layer_bwd_gates, engine.mask_step, explain.learn_mask, explain.mask_selection):
        assert callable(f)
