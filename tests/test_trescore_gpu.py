"""The temporal RDigraph.rescore, quadruple fact masks and T_RED_GNN.fidelity on the MI355X (-m gpu), on temporal_ref.hand_graph():
against the float64 numpy reference of tests/trescore_ref.py (the walk's arithmetic over the explicit edge list), against the model's
own forward on a model rebuilt from the quadruples without the deleted ones, and the properties of the fidelity measures.  The rows
and the deleted quadruples are trescore_ref's (tests/test_trescore_ref.py asserts their conditions with the reference alone).
Tolerance: the project's stated one through tests/_util.assert_close_fp32, rtol 1e-4 and atol 2e-5 of the fp64 reference, or 4x the
fp32 reference's own error."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import temporal_ref as TR
from tests import trescore_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
N_ENT, N_ROWS_TAB, N_TIME = TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1, TR.HAND_N_TIME
M = R.INVERSE_OFFSET
CONFIGS = [(16, 3, "idd", 2, False), (20, 5, "tanh", 3, False), (64, 5, "relu", 3, True), (128, 10, "relu", 2, False)]   # (d, a, act, L, shared)


def _model(quads, d, a, act, L, shared, state=None):
    return TR.make_model(quads, N_ENT, N_ROWS_TAB, N_TIME, L, d, a, act, shared=shared, state=state)


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


@pytest.mark.parametrize("d,a,act,L,shared", CONFIGS)
def test_rescore_against_the_reference_and_the_rebuilt_model(d, a, act, L, shared):
    quads, heads, rels, times, objs, deleted = R.inputs(L)
    model = _model(quads, d, a, act, L, shared)
    batch = {"head": heads, "relation": rels, "time": times}
    B = len(heads)
    rd = model.explain(batch, objs)
    e, t = rd.edges.cpu().numpy().astype(np.int64), rd.time.cpu().numpy().astype(np.int64)
    want_e, want_t, want_reached = R.digraph_of(quads, heads, objs, L)
    assert np.array_equal(U.sorted_edges(np.column_stack([e, t])), U.sorted_edges(np.column_stack([want_e, want_t])))
    assert np.array_equal(rd.reached.cpu().numpy(), want_reached) and want_reached.all()
    assert rd.n_rel == model.n_rel == R.IDENTITY and rd.n_time == N_TIME and rd.data_row is None
    assert rd.q_sub.dtype == rd.q_rel.dtype == torch.int64 and rd.q_sub.tolist() == heads.tolist() and rd.q_rel.tolist() == rels.tolist()
    p = TR.state_of(model)
    ref = lambda keep, dt: R.rescore(p, e, t, heads, rels, times, N_ENT, L, act, keep=keep, shared_tables=shared, dtype=dt)
    tag = "d%d a%d %s L%d shared=%s" % (d, a, act, L, shared)

    # ---- every edge kept: the model's own score
    rs = rd.rescore(model)
    _compare(tag + " keep=None", rs, ref(None, np.float64), ref(None, np.float32))
    assert bool(rs.live.all()) and bool(rs.reached.all())
    np.testing.assert_allclose(rs.score.cpu().numpy(), rd.score.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)   # two fp32 evaluations
    first = rd.edges[:, 1] == 1
    assert int(first.sum()) > B and torch.equal(rs.alpha[first], rd.alpha[first])         # hop 1: the forward's float, bit for bit
    again = rd.rescore(model, keep=torch.ones(len(e), dtype=torch.uint8, device="cuda"))
    assert torch.equal(again.score, rs.score) and torch.equal(again.alpha, rs.alpha)
    host = rd.rescore(model, keep=np.ones(len(e), np.uint8))
    assert torch.equal(host.score, rs.score) and torch.equal(host.alpha, rs.alpha)
    was_training = model.training
    model.train()
    try:
        assert torch.equal(rd.rescore(model).score, rs.score) and model.training           # eval semantics, and the flag comes back
    finally:
        model.train(was_training)

    # ---- the quadruples deleted, with their inverse twins, at every hop
    m = rd.fact_mask(deleted, inverse_offset=M)
    assert np.array_equal(m.cpu().numpy(), R.fact_mask(e, t, R.IDENTITY, deleted, inverse_offset=M))
    dup = (e[:, 2] == 3) & (e[:, 3] == 0) & (e[:, 4] == 0) & (t == 2) & (e[:, 0] == 1) & (e[:, 1] == 1)
    assert dup.sum() == 2 and m.cpu().numpy()[dup].all()                                  # both copies of the duplicate go
    keep = ~m
    rs = rd.rescore(model, keep=keep)
    k_h = keep.cpu().numpy()
    assert torch.equal(rd.rescore(model, keep=k_h.astype(np.uint8)).score, rs.score)      # a host array goes along, bits unchanged
    r64, r32 = ref(k_h, np.float64), ref(k_h, np.float32)
    reached = r64[1]
    print("%s: %d quadruples deleted, %d of %d edges kept, %d live, %d of %d rows reached" % (tag, len(deleted), k_h.sum(), len(e),
                                                                                           r64[2].sum(), reached.sum(), B))
    assert 4 * reached.sum() >= B and (~reached).any(), "the inputs must leave a quarter of the rows reached and cut one off"
    assert (k_h & ~r64[2]).any(), "the inputs must leave kept edges dangling"
    _compare(tag + " quadruples deleted", rs, r64, r32)

    # ---- ... is the model's forward on the quadruple graph without them
    cut = R.without_quads(quads, deleted, M)
    assert len(cut) == len(quads) - 2 * len(deleted) - 2
    rebuilt = _model(cut, d, a, act, L, shared, state=TR.state_of(model))
    with torch.no_grad():
        fwd = rebuilt(batch, mode="test")[np.arange(B), objs].cpu().numpy()
    assert np.array_equal(fwd != 0, reached), tag + ": the forward on the rebuilt graph reaches other rows"
    U.assert_close_fp32(fwd, r32[0], r64[0], RTOL, ATOL, tag + " forward on the rebuilt graph")
    # (two fp32 evaluations of one number, each within the tolerance of it)
    np.testing.assert_allclose(rs.score.cpu().numpy(), fwd, rtol=2 * RTOL, atol=2 * ATOL)


def test_rescore_refuses_other_models_and_modes():
    """With the tensors on the device the checks are those of tests/test_tfidelity_host.py: nothing is launched."""
    quads, heads, rels, times, objs, _ = R.inputs(2)
    model = _model(quads, 16, 3, "idd", 2, False)
    rd = model.explain({"head": heads, "relation": rels, "time": times}, objs)
    with pytest.raises(ValueError, match="temporal.*mode must be 'test'"):
        rd.rescore(model, mode="valid")
    with pytest.raises(ValueError, match="temporal.*n_layer=3"):
        rd.rescore(_model(quads, 16, 3, "idd", 3, False))
    with pytest.raises(ValueError, match="temporal.*missing: n_time"):
        type(rd)(**{**rd.__dict__, "n_time": None}).rescore(model)
    with pytest.raises(ValueError, match="out of range"):
        bad = rd.edges.clone()
        bad[0, 4] = N_ENT
        type(rd)(**{**rd.__dict__, "edges": bad}).rescore(model)
    with pytest.raises(ValueError, match=r"\[F, 4\]"):
        rd.fact_mask([(3, 0, 0)])


def test_fidelity_columns_are_rescores_of_the_path_masks():
    quads, heads, rels, times, objs, _ = R.inputs(2)
    d, a, act, L, shared = CONFIGS[0]
    k, B = 3, len(heads)
    model = _model(quads, d, a, act, L, shared)
    batch = {"head": heads, "relation": rels, "time": times}
    f = model.fidelity(batch, objs, k=k, inverse_offset=M)
    rd, paths = f.paths.digraph, f.paths
    assert f.score is rd.score and f.without.shape == f.only.shape == f.reached_without.shape == f.reached_only.shape == (B, k)
    assert torch.equal(f.count, paths.count) and paths.edge.shape[1] == k
    loops = rd.edges[:, 3] == model.n_rel
    assert int(loops.sum()) > 0 and bool((rd.time[loops] == N_TIME - 1).all())
    for j in range(k):
        m = paths.fact_mask(j + 1, inverse_offset=M)
        assert not bool((m & loops).any())
        wo, on = rd.rescore(model, keep=~m), rd.rescore(model, keep=m | loops)
        assert torch.equal(f.without[:, j], wo.score) and torch.equal(f.reached_without[:, j], wo.reached)
        assert torch.equal(f.only[:, j], on.score) and torch.equal(f.reached_only[:, j], on.reached)
    # the mask of the paths' quadruples is the reference's, every quadruple for its own row
    at = paths.edge[:, :k].reshape(-1)
    at = at[at >= 0].cpu().numpy()
    e, t = rd.edges.cpu().numpy().astype(np.int64), rd.time.cpu().numpy().astype(np.int64)
    want = R.fact_mask(e, t, R.IDENTITY, np.column_stack([e[at, 2:5], t[at]]), rows=e[at, 0], inverse_offset=M)
    assert np.array_equal(paths.fact_mask(k, inverse_offset=M).cpu().numpy(), want)
    plain = paths.fact_mask(k).cpu().numpy()                                  # without the twins: the steps' own quadruples, a subset
    assert np.array_equal(plain, R.fact_mask(e, t, R.IDENTITY, np.column_stack([e[at, 2:5], t[at]]), rows=e[at, 0])) and (plain <= want).all()
    assert torch.equal(f.necessity(), f.score[:, None] - f.without) and torch.equal(f.sufficiency_gap(), f.score[:, None] - f.only)
    assert len(f.format()) == B
    count = f.count.cpu().numpy()
    rw = f.reached_without.cpu().numpy()
    print("paths per row %s; reached without the best j paths: %s of %d" % (count.tolist(), rw.sum(0).tolist(), B))
    # the inputs: both outcomes of the deletion occur, and some row has no more than k paths in all
    assert rw.any() and (~rw).any()
    total = rd.top_paths(k + 1).count.cpu().numpy()
    few = np.nonzero((total <= k) & (total >= 1))[0]
    assert len(few) >= 2 and (count[few] == total[few]).all()
    # for j past count a row repeats its value at j = count
    for b in range(B):
        for j in range(max(count[b], 1), k):
            assert f.without[b, j] == f.without[b, count[b] - 1 if count[b] else 0] and f.only[b, j] == f.only[b, max(count[b] - 1, 0)]
    # a row whose digraph has at most k paths: those paths' quadruples and the self-loops are the whole digraph, ``only`` is the score
    p = TR.state_of(model)
    s64 = R.rescore(p, e, t, heads, rels, times, N_ENT, L, act)[0]
    s32 = R.rescore(p, e, t, heads, rels, times, N_ENT, L, act, dtype=np.float32)[0]
    only_at_count = f.only.cpu().numpy()[few, count[few] - 1]
    U.assert_close_fp32(only_at_count, s32[few], s64[few], RTOL, ATOL, "only at j = count")
    np.testing.assert_allclose(only_at_count, f.score.cpu().numpy()[few], rtol=2 * RTOL, atol=2 * ATOL)
    assert f.reached_only.cpu().numpy()[few, count[few] - 1].all()
    # objs=None: batch["tail"] where the batch has it
    g = model.fidelity({**batch, "tail": objs}, k=1, inverse_offset=M)
    assert torch.equal(g.paths.digraph.edges, rd.edges) and torch.equal(g.without[:, 0], f.without[:, 0]) and torch.equal(g.only[:, 0], f.only[:, 0])


def test_fidelity_all_is_independent_of_the_batching():
    quads = TR.hand_graph()
    model = _model(quads, 16, 3, "relu", 2, False)
    base = quads[quads[:, 1] != R.IDENTITY]
    pick = base[np.random.default_rng(3).choice(len(base), 40, replace=False)]
    out = model.fidelity_all(pick, k=2, batch_size=16, inverse_offset=M)
    assert out["n"] == 40 and out["k"] == 2
    for key in ("necessity_mean", "necessity_median", "sufficiency_gap_mean", "sufficiency_gap_median", "disconnected"):
        assert len(out[key]) == 2 and all(np.isfinite(v) for v in out[key]), key
    assert all(0.0 <= v <= 1.0 for v in out["disconnected"]) and out["disconnected"][0] <= out["disconnected"][1]
    assert out["disconnected"][1] > 0.0                                        # a leaf's only link deleted: the answer is cut off
    one = model.fidelity_all(torch.as_tensor(pick), k=2, batch_size=40, inverse_offset=M)
    assert one["disconnected"] == out["disconnected"]
    for key in ("necessity_mean", "sufficiency_gap_mean"):
        np.testing.assert_allclose(one[key], out[key], rtol=1e-5, atol=1e-6)
