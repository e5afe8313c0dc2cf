"""tests/extrap_ref.py without a GPU: the float64 walk's logits and node sets against the oracle's extrap_forward in float64 on the
graph of the GPU tests, the shape of its hops, and segment_topk_ref on a hand-made segment."""
import numpy as np
import pytest
import torch

from oracle import redgnn_oracle as orc
from tests import extrap_ref as R


def _state(d, a, n_layer, seed=3):
    """Random parameters with the model's names and shapes (the model itself needs the device for its graph)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64) * 0.3
    p = {"linear_classifier.weight": r(1, d), "linear_classifier.bias": r(1), "past_linear.weight": r(d, d),
         "time_embed.periodic.weight": r(1, 48) * 0.03}
    for name in ("linear_neg", "linear_pos"):
        p["time_embed.%s.weight" % name], p["time_embed.%s.bias" % name] = r(1, 96, d), r(1, d)
    for i in range(n_layer):
        p["rela_embed_layer.%d.weight" % i] = r(R.N_REL + 2, d)
        p["attention_1_layer.%d.weight" % i], p["attention_2_layer.%d.weight" % i] = r(a, 3 * d), r(1, a)
    return p


@pytest.mark.parametrize("d,a,act,n_layer,B", R.CASES + [(32, 30, "relu", 4, 5)])
def test_walk_equals_the_oracle_in_float64(d, a, act, n_layer, B):
    data, q = R.make_case(d, B)
    assert (data[10:14] == data[9]).all() and len(np.unique(data[:, 3] // 24)) < 220
    off = orc.get_time_offset_list(data, 24)
    p = _state(d, a, n_layer)
    logits, nodes, hops, cur_t = R.walk(p, data, off, 24, R.N_ENT, R.N_REL, q[:, 0], q[:, 1], q[:, 3], n_layer, act)
    ref_s, _, ref_nodes = orc.extrap_forward(p, data, off, 24, R.N_ENT, R.N_REL, q[:, 0], q[:, 1], q[:, 3], n_layer, act, dtype=torch.float64)
    assert np.array_equal(nodes, ref_nodes)
    np.testing.assert_allclose(logits, ref_s.numpy()[nodes[:, 0], nodes[:, 1]], rtol=1e-9, atol=1e-11)
    assert cur_t.min() < R.WINDOW < cur_t.max()                  # queries older and younger than the window
    lo, hi = off[np.maximum(cur_t - R.WINDOW, 0)], off[cur_t]
    for e, al, day in hops:
        loop = e[:, 4] < 0
        assert loop.any() and (~loop).any() and ((al >= 0) & (al <= 1)).all()
        assert (e[loop, 1] == e[loop, 3]).all() and (e[loop, 2] == R.N_REL).all()
        rows = e[~loop]
        assert np.array_equal(data[rows[:, 4], :3], rows[:, 1:4])
        assert ((rows[:, 4] >= lo[rows[:, 0]]) & (rows[:, 4] < hi[rows[:, 0]])).all()
        assert (day[~loop] == data[rows[:, 4], 3] // 24).all() and (day[loop] == np.maximum(cur_t - R.WINDOW, 0)[e[loop, 0]]).all()


def test_segment_topk_ref_on_a_hand_made_batch():
    sc = np.array([0.5, -0.0, 0.0, 2.0, np.nan, 0.5, 1.0, -np.inf], np.float32)
    ent = np.array([4, 9, 2, 7, 1, 3, 8, 0])
    known = (np.array([5, 11], np.int64), np.array([0, 2, 3], np.int64), np.array([7, 100, 8], np.int32))
    ids, val, prob = R.segment_topk_ref(sc, ent, [0, 6, 6, 8], 4, np.array([5, 11, 6]), known)
    assert ids.tolist() == [[3, 4, 2, 9], [-1] * 4, [8, 0, -1, -1]]           # 7 is known for key 5; key 6 is absent: nothing hidden
    assert np.signbit(val[0]).tolist() == [False, False, False, True] and val[2].tolist()[:2] == [1.0, -np.inf]
    assert np.isnan(prob[0]).all() and (prob[1] == 0).all() and prob[2].tolist() == [1.0, 0.0, 0.0, 0.0]
    ids, val, prob = R.segment_topk_ref(sc[:4], ent[:4], [0, 4], 2)
    assert ids.tolist() == [[7, 4]] and abs(prob.sum() - (np.exp(0) + np.exp(-1.5)) / (1 + np.exp(-1.5) + 2 * np.exp(-2))) < 1e-12
