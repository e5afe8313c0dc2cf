"""CPU-only checks of the extrapolation model's predict / explain: the new optional fields of Prediction and RDigraph, RDigraph.lag,
the C-ABI entry points declared, bound and exported, and the argument checks of T_RED_GNN.predict / explain, which run before any
device work (the model here is a namespace with the attributes the checks read: nothing else may be touched)."""
import types

import numpy as np
import pytest
import torch


def test_new_result_fields_default_to_none():
    from red_gnn_amd.explain import RDigraph
    from red_gnn_amd.prediction import Prediction
    p = Prediction(ids=torch.zeros((1, 2), dtype=torch.int64), scores=torch.zeros((1, 2)))
    assert p.prob is None
    rd = RDigraph(edges=torch.zeros((0, 5), dtype=torch.int32), alpha=torch.zeros(0), offsets=torch.zeros(2, dtype=torch.int64),
                  reached=torch.zeros(1, dtype=torch.bool), score=torch.zeros(1), n_hops=2)
    assert rd.data_row is None and rd.time is None and rd.q_time is None
    with pytest.raises(ValueError):
        rd.lag()
    with pytest.raises(ValueError):
        rd.direction()


def test_lag_on_a_hand_made_digraph():
    from red_gnn_amd.explain import RDigraph
    edges = torch.tensor([[0, 1, 4, 6, 4], [0, 1, 4, 2, 7], [0, 2, 7, 0, 9], [1, 1, 3, 6, 3], [1, 2, 3, 1, 9]], dtype=torch.int32)
    rd = RDigraph(edges=edges, alpha=torch.ones(5), offsets=torch.tensor([0, 3, 5]), reached=torch.ones(2, dtype=torch.bool),
                  score=torch.zeros(2), n_hops=2, time=torch.tensor([80, 150, 199, 0, 17], dtype=torch.int32),
                  q_time=torch.tensor([200, 20], dtype=torch.int32), data_row=torch.tensor([-1, 40, 99, -1, 3], dtype=torch.int32))
    lag = rd.lag()
    assert lag.dtype == torch.int32 and lag.tolist() == [120, 50, 1, 20, 3]


def test_entry_points_are_declared_and_bound():
    import os
    import re
    from red_gnn_amd import _lib, engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "redgnn.h")).read()
    for name in ("rg_segment_topk", "rg_xexplain_count", "rg_xexplain_emit"):
        assert re.search(r"\bint %s\(" % name, header) and name in _lib.SYMBOLS
    src = open(os.path.join(root, "red-gnn_amd", "csrc", "segment_topk.hip")).read()
    assert int(re.search(r"SEG_STAGE_MAX = (\d+);", src).group(1)) == engine.SEGMENT_TOPK_STAGE_MAX
    assert int(re.search(r"SEG_LIST_LDS = (\d+);", src).group(1)) == engine.SEGMENT_TOPK_LIST_LDS


def _model():
    return types.SimpleNamespace(n_ent=20, n_rel_true=4, time_granularity=24, time_offset_list=np.zeros(12, np.int64))


def _batch(src, rel, ts):
    return types.SimpleNamespace(src_idx=np.asarray(src), rel_idx=np.asarray(rel), ts=np.asarray(ts))


BAD_BATCHES = [
    _batch([1.0, 2.0], [0, 1], [24, 48]),            # float ids
    _batch([1, 2], [0.5, 1.0], [24, 48]),
    _batch([1, 2], [0, 1], [24.0, 48.0]),
    _batch([True, False], [0, 1], [24, 48]),
    _batch([1, 2], [0], [24, 48]),                   # lengths
    _batch([1, 2], [0, 1], [24]),
    _batch([], [], []),
    _batch([1, 20], [0, 1], [24, 48]),               # ranges
    _batch([-1, 2], [0, 1], [24, 48]),
    _batch([1, 2], [0, 4], [24, 48]),
    _batch([1, 2], [-1, 1], [24, 48]),
    _batch([1, 2], [0, 1], [24, 12 * 24]),
    _batch([1, 2], [0, 1], [-1, 48]),
]


def test_predict_rejects_bad_arguments_before_any_device_work():
    from red_gnn_amd import extrapolation as X
    good = _batch([1, 2], [0, 3], [24, 11 * 24 + 23])
    for k in (0, 1025, -1, 1.0, "3", True, None):
        with pytest.raises(ValueError):
            X.T_RED_GNN.predict(_model(), good, k=k)
    for bad in BAD_BATCHES:
        with pytest.raises(ValueError):
            X.T_RED_GNN.predict(_model(), bad, k=3)
    with pytest.raises(AttributeError):              # a good call gets past the checks (the namespace has no parameters)
        X.T_RED_GNN.predict(_model(), good, k=3)


def test_explain_rejects_bad_arguments_before_any_device_work():
    from red_gnn_amd import extrapolation as X
    good = _batch([1, 2], [0, 3], [24, 11 * 24 + 23])
    for bad in BAD_BATCHES:
        with pytest.raises(ValueError):
            X.T_RED_GNN.explain(_model(), bad, [0, 1])
    for objs in ([0], [0, 1, 2], [0, 20], [-1, 0], [0.0, 1.0]):
        with pytest.raises(ValueError):
            X.T_RED_GNN.explain(_model(), good, objs)
    with pytest.raises(ValueError):
        X.T_RED_GNN.explain(_model(), good, [0, 1], min_alpha=float("nan"))
    with pytest.raises(AttributeError):
        X.T_RED_GNN.explain(_model(), good, [0, 1])
