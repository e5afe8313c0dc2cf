"""CPU tests of the temporal explain / profile / predict support: the float64 reference walk (tests/temporal_ref.py) pinned to the oracle
and to the reference-produced fixture, and the host logic of the feature (temporal_known_index, the four-axis AttentionProfile,
RDigraph.direction).

The walk and the oracle both compute in float64 but sum in different orders (per-edge loops here, torch index_add_ / matmul there), so
their scores agree to float64 rounding, not bit for bit: a few thousand operations of relative error 1.1e-16 each on values of order
1 stay below RTOL64, ATOL64 = 1e-10, 1e-12, six orders of magnitude under the float32 tolerances the GPU tests use."""
import numpy as np
import pytest
import torch

from oracle import redgnn_oracle as orc
from tests import _util as U
from tests import layer_ref as LR
from tests import temporal_ref as TR

RTOL, ATOL = 1e-4, 1e-5                  # tests/test_oracle_golden.py's for the fixture
RTOL64, ATOL64 = 1e-10, 1e-12


def random_params(rng, n_rela_rows, n_time, n_layer, d, a, shared=False):
    """A T_RED_GNN state dict (the parameters the forward reads) of seeded normal values."""
    f = lambda *shape: torch.tensor(rng.standard_normal(shape) * 0.3, dtype=torch.float32)
    p = {"time_embed.weight": f(n_time, d), "past_linear.weight": f(d, d), "now_linear.weight": f(d, d),
         "future_linear.weight": f(d, d), "linear_classifier.weight": f(1, d), "linear_classifier.bias": f(1)}
    if shared:
        p.update({"rela_embed.weight": f(n_rela_rows, d), "attention_1.weight": f(a, 3 * d), "attention_2.weight": f(1, a)})
    else:
        for i in range(n_layer):
            p.update({"rela_embed_layer.%d.weight" % i: f(n_rela_rows, d), "attention_1_layer.%d.weight" % i: f(a, 3 * d),
                      "attention_2_layer.%d.weight" % i: f(1, a)})
    return p


def test_walk_matches_oracle_and_reference_fixture():
    fx = U.load("temporal_model_py.npz")
    n_layer = int(fx["cfg"][0])
    p = U.params_of(fx)
    s, hops, nodes = TR.walk(p, fx["quads"], int(fx["n_ent"]), fx["heads"], fx["rels"], fx["times"], n_layer, str(fx["act"]),
                             shared_tables=True)
    trace = []
    ref = orc.temporal_forward(p, fx["quads"], int(fx["n_ent"]), fx["heads"], fx["rels"], fx["times"], n_layer, str(fx["act"]),
                               shared_tables=True, dtype=torch.float64, trace=trace).numpy()
    np.testing.assert_allclose(s, ref, rtol=RTOL64, atol=ATOL64)
    assert np.array_equal(s == 0, ref == 0)
    assert [len(e) for e, _ in hops] == [t["n_edges"] for t in trace] and np.array_equal(nodes, trace[-1]["nodes"])
    np.testing.assert_allclose(s, fx["scores"], rtol=RTOL, atol=ATOL)           # the reference's own output
    assert np.array_equal(s == 0, fx["scores"] == 0)
    for e, al in hops:
        assert e.shape[1] == 5 and len(al) == len(e) and (al > 0).all() and (al < 1).all()


@pytest.mark.parametrize("act,n_layer", [("relu", 2), ("tanh", 3)])
def test_walk_matches_oracle_on_a_layer_case(act, n_layer):
    c = LR._temporal_case("ref", seed=5, B=9)
    p = random_params(np.random.default_rng(1), c.n_rela_rows, c.n_time, n_layer, 20, 5)
    heads, rels = c.nodes0[:, 1], np.arange(c.B) % c.n_rela_rows
    s, hops, _ = TR.walk(p, c.quads, c.n_ent, heads, rels, c.q_time, n_layer, act)
    ref = orc.temporal_forward(p, c.quads, c.n_ent, heads, rels, c.q_time, n_layer, act, dtype=torch.float64).numpy()
    np.testing.assert_allclose(s, ref, rtol=RTOL64, atol=ATOL64)
    assert np.array_equal(s == 0, ref == 0)
    d_all = np.concatenate([TR.direction(e[:, 4], c.q_time[e[:, 0]]) for e, _ in hops])
    assert set(d_all.tolist()) == {0, 1, 2}


# ---- temporal_known_index -----------------------------------------------------------------------------------------------------------
def test_temporal_known_index_against_a_python_loop():
    from red_gnn_amd.prediction import temporal_known_index
    rng = np.random.default_rng(0)
    n_ent, R, T = 17, 5, 4
    quads = np.stack([rng.integers(0, n_ent, 400), rng.integers(0, R, 400), rng.integers(0, n_ent, 400), rng.integers(0, T, 400)], 1)
    quads = np.concatenate([quads, quads[:30]], 0)                      # exact duplicates
    keys, ptr, idx = temporal_known_index(quads, R, T)
    want = {}
    for h, r, t, tm in quads.tolist():
        want.setdefault((h * R + r) * T + tm, set()).add(t)
    assert keys.dtype == np.int64 and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert keys.tolist() == sorted(want) and len(ptr) == len(keys) + 1 and ptr[0] == 0 and ptr[-1] == len(idx)
    for i, k in enumerate(keys.tolist()):
        assert idx[ptr[i]:ptr[i + 1]].tolist() == sorted(want[k])
    keys, ptr, idx = temporal_known_index(np.zeros((0, 4), np.int64), R, T)
    assert len(keys) == 0 and ptr.tolist() == [0] and len(idx) == 0
    keys, ptr, idx = temporal_known_index([[3, 2, 1, 0]], R, T)
    assert keys.tolist() == [(3 * R + 2) * T] and ptr.tolist() == [0, 1] and idx.tolist() == [1]
    with pytest.raises(ValueError):
        temporal_known_index([[0, R, 1, 0]], R, T)
    with pytest.raises(ValueError):
        temporal_known_index([[0, 0, 1, T]], R, T)


# ---- AttentionProfile with a direction axis ---------------------------------------------------------------------------------------------
AXES4 = ("group", "hop", "direction", "relation")


def _profile4():
    from red_gnn_amd.profile import AttentionProfile
    one = 1 << 32
    count = torch.zeros((2, 2, 3, 4), dtype=torch.int64)
    fixed = torch.zeros((2, 2, 3, 4), dtype=torch.int64)
    # row 0, hop 0: relation 1 has 2 past edges (alpha sum 1.0) and 1 future edge (0.25); relation 2 has 1 "now" edge (0.75);
    # relation 3 has 4 past edges (alpha sum 1.0)
    count[0, 0, 0, 1], fixed[0, 0, 0, 1] = 2, one
    count[0, 0, 2, 1], fixed[0, 0, 2, 1] = 1, one // 4
    count[0, 0, 1, 2], fixed[0, 0, 1, 2] = 1, 3 * one // 4
    count[0, 0, 0, 3], fixed[0, 0, 0, 3] = 4, one
    # row 0, hop 1: relation 0 has 1 future edge (0.5)
    count[0, 1, 2, 0], fixed[0, 1, 2, 0] = 1, one // 2
    # row 1, hop 1: relation 3 has 3 past edges (alpha sum 1.5)
    count[1, 1, 0, 3], fixed[1, 1, 0, 3] = 3, 3 * one // 2
    return AttentionProfile(fixed, count, "query", AXES4)


def test_four_axis_profile_collapse_total_add_top():
    prof = _profile4()
    assert prof.n_hops == 2 and prof.alpha_sum.shape == (2, 2, 3, 4) and prof.alpha_sum[0, 0, 0, 1].item() == 1.0
    m = prof.mean()
    assert m[0, 0, 0, 1].item() == 0.5 and m[0, 0, 0, 3].item() == 0.25 and torch.isnan(m[1, 0, 0, 0])
    c = prof.collapse("direction")
    assert c.axes == ("group", "hop", "relation") and c.count.shape == (2, 2, 4) and c.group == "query"
    assert c.count[0, 0].tolist() == [0, 3, 1, 4] and c.fixed[0, 0].tolist() == [0, (1 << 32) * 5 // 4, 3 * (1 << 32) // 4, 1 << 32]
    assert torch.equal(c.count, prof.count.sum(2)) and torch.equal(c.fixed, prof.fixed.sum(2))
    for name in ("time", "hop", "group", "relation"):                     # only an added axis can be summed away
        with pytest.raises(ValueError):
            prof.collapse(name)
    with pytest.raises(ValueError):
        c.collapse("direction")                                          # already gone
    t = prof.total()
    assert t.axes == AXES4 and t.count.shape == (2, 1, 3, 4) and t.count[0, 0, 2].tolist() == [1, 1, 0, 0]
    assert torch.equal(t.collapse("direction").count, c.total().count)
    two = prof + prof
    assert two.axes == AXES4 and torch.equal(two.count, 2 * prof.count) and torch.equal(two.fixed, 2 * prof.fixed)
    with pytest.raises(ValueError):
        prof + c                                                         # different axes do not add
    assert prof.cpu().axes == AXES4
    # top: all directions (relation 2: 0.75, relation 1: 1.25 / 3, relation 3: 0.25), then one direction
    ids, mean = prof.top(0, k=3)
    assert ids.tolist() == [[2, 1, 3], [0, -1, -1]]
    assert mean[0].tolist() == [0.75, 1.25 / 3, 0.25] and mean[1, 0].item() == 0.5 and torch.isnan(mean[1, 1:]).all()
    ids_c, mean_c = c.top(0, k=3)
    assert torch.equal(ids, ids_c) and torch.equal(mean.nan_to_num(-1), mean_c.nan_to_num(-1))
    ids, mean = prof.top(0, k=2, direction=0)                            # past: relation 1 (0.5), relation 3 (0.25)
    assert ids.tolist() == [[1, 3], [-1, -1]] and mean[0].tolist() == [0.5, 0.25]
    ids, mean = prof.top(0, k=2, direction=1)                            # now: relation 2 only
    assert ids.tolist() == [[2, -1], [-1, -1]] and mean[0, 0].item() == 0.75
    ids, mean = prof.top(0, k=1, direction=2)                            # future: relation 1 (0.25); hop 2: relation 0 (0.5)
    assert ids.tolist() == [[1], [0]] and mean.reshape(-1).tolist() == [0.25, 0.5]
    for bad in (3, -1, True, 1.0, "past"):
        with pytest.raises(ValueError):
            prof.top(0, k=1, direction=bad)


def test_three_axis_profile_is_unchanged():
    from red_gnn_amd.profile import AttentionProfile
    one = 1 << 32
    count = torch.tensor([[[2, 0, 1], [0, 4, 0]]], dtype=torch.int64)           # [1, 2, 3]
    fixed = torch.tensor([[[one, 0, one // 4], [0, one, 0]]], dtype=torch.int64)
    prof = AttentionProfile(fixed, count, "query")
    assert prof.axes == ("group", "hop", "relation") and prof.n_hops == 2
    assert prof.alpha_sum.tolist() == [[[1.0, 0.0, 0.25], [0.0, 1.0, 0.0]]]
    m = prof.mean()
    assert m[0, 0, 0].item() == 0.5 and m[0, 0, 2].item() == 0.25 and m[0, 1, 1].item() == 0.25 and torch.isnan(m[0, 0, 1])
    t = prof.total()
    assert t.count.tolist() == [[[2, 4, 1]]] and t.fixed.tolist() == [[[one, one, one // 4]]] and t.axes == prof.axes
    ids, mean = prof.top(0, k=2)
    assert ids.tolist() == [[0, 2], [1, -1]] and mean[0].tolist() == [0.5, 0.25] and mean[1, 0].item() == 0.25 and torch.isnan(mean[1, 1])
    ids2, mean2 = prof.top(0, k=2, direction=None)
    assert torch.equal(ids, ids2)
    with pytest.raises(ValueError):
        prof.top(0, k=2, direction=1)
    assert torch.equal((prof + prof).count, 2 * count)
    with pytest.raises(ValueError):
        prof.collapse("hop")
    with pytest.raises(ValueError):
        prof.collapse("direction")


# ---- batch validation and the eval-mode context of the temporal drivers ------------------------------------------------------------------
def test_batch_ids_and_eval_semantics():
    import types
    from red_gnn_amd.temporal import batch_ids, eval_semantics
    m = types.SimpleNamespace(n_ent=10, n_rel=4, n_time=6)
    h, r, t = batch_ids(m, {"head": [1, 9], "relation": torch.tensor([0, 4]), "time": np.array([5, 0], np.int32)}, "x")
    assert h.tolist() == [1, 9] and r.tolist() == [0, 4] and t.tolist() == [5, 0] and h.dtype == r.dtype == t.dtype == np.int64
    ok = {"head": [1], "relation": [0], "time": [0]}
    for bad in ({"head": [1.7]}, {"relation": [True]}, {"time": torch.tensor([1.0])}, {"head": [10]}, {"relation": [5]}, {"time": [6]},
                {"head": [-1]}, {"head": [1, 2]}, {"head": [], "relation": [], "time": []}):
        with pytest.raises(ValueError):
            batch_ids(m, {**ok, **bad}, "x")
    with pytest.raises(ValueError):
        batch_ids(m, {"head": [1], "relation": [0]}, "x")
    net = torch.nn.Sequential(torch.nn.Dropout(0.5), torch.nn.Sequential(torch.nn.Dropout(0.5)))
    net.train()
    net[0].eval()                                                        # a submodule set on its own, under a training root
    with eval_semantics(net):
        assert not any(x.training for x in net.modules())
    assert net.training and not net[0].training and net[1].training and net[1][0].training
    net.eval()
    with eval_semantics(net):
        pass
    assert not any(x.training for x in net.modules())


# ---- RDigraph.direction -------------------------------------------------------------------------------------------------------------
def test_rdigraph_direction():
    from red_gnn_amd.explain import RDigraph
    edges = torch.tensor([[0, 1, 5, 0, 6], [0, 1, 5, 0, 6], [0, 2, 6, 1, 7], [1, 1, 2, 0, 3], [1, 2, 3, 1, 4]], dtype=torch.int32)
    time = torch.tensor([2, 9, 5, 0, 7], dtype=torch.int32)
    q_time = torch.tensor([5, 0], dtype=torch.int32)
    rd = RDigraph(edges=edges, alpha=torch.ones(5), offsets=torch.tensor([0, 3, 5]), reached=torch.tensor([True, True]),
                  score=torch.zeros(2), n_hops=2, time=time, q_time=q_time)
    d = rd.direction()
    assert d.dtype == torch.int8 and d.tolist() == [0, 2, 1, 1, 2]
    assert d.tolist() == TR.direction(time.numpy(), q_time.numpy()[edges[:, 0].numpy()]).tolist()
    static = RDigraph(edges=edges, alpha=torch.ones(5), offsets=torch.tensor([0, 3, 5]), reached=torch.tensor([True, True]),
                      score=torch.zeros(2), n_hops=2)
    assert static.time is None and static.q_time is None
    with pytest.raises(ValueError):
        static.direction()
    empty = RDigraph(edges=edges[:0], alpha=torch.ones(0), offsets=torch.tensor([0, 0, 0]), reached=torch.tensor([False, False]),
                     score=torch.zeros(2), n_hops=2, time=time[:0], q_time=q_time)
    assert empty.direction().shape == (0,)
