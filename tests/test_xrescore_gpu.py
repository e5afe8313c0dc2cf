"""RDigraph.rescore, fact_mask and data_row_mask on extrapolation r-digraphs and extrapolation.T_RED_GNN.fidelity / fidelity_all on the
MI355X (-m gpu), on extrap_ref.make_case: against the float64 numpy reference of tests/xrescore_ref.py (the walk's arithmetic over the
explicit edge list), against the model's own forward on a model rebuilt from the data without the deleted rows, and the properties of
the fidelity measures.  The rows and the deleted facts are xrescore_ref's (tests/test_xrescore_ref.py asserts their conditions with the
reference alone).  Tolerance: the project's stated one through tests/_util.assert_close_fp32, rtol 1e-4 and atol 2e-5 of the fp64
reference, or 4x the fp32 reference's own error; integers, masks, ``reached`` and ``live`` exact."""
import functools

import numpy as np
import pytest
import torch

from tests import _util as U
from tests import extrap_ref as XR
from tests import xrescore_ref as R
from tests.temporal_ref import state_of

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
CASES = XR.CASES + [(32, 30, "relu", 4, 5)]


@functools.lru_cache(maxsize=None)
def _setup(d, a, act, L, B):
    """Model, data, queries, rows (query, answer) and the digraph explain returns for them."""
    from red_gnn_amd import extrapolation as X
    data, q = XR.make_case(d, B)
    q = R.queries_of_case(data, q)
    model = XR.make_model(data, d, a, act, L)
    off = X.get_time_offset_list(data, 24)
    _, last, hops, cur_t = XR.walk(state_of(model), data, off, 24, XR.N_ENT, XR.N_REL, q[:, 0], q[:, 1], q[:, 3], L, act)
    q_of, objs = R.rows_of_case(q, hops, last, data)
    rows = q[q_of]
    rd = model.explain(XR.Batch(rows), objs)
    return model, data, rows, objs, cur_t[q_of], rd


def _compare(tag, rs, ref64, ref32):
    score, reached, live, alpha = ref64
    assert np.array_equal(rs.reached.cpu().numpy(), reached), tag + ": reached"
    assert rs.live.dtype == torch.bool and np.array_equal(rs.live.cpu().numpy(), live), tag + ": live"
    got = rs.score.cpu().numpy()
    assert (got[~reached] == 0).all(), tag + ": an unreached row does not score exactly 0"
    print("%s: max |score - ref64| %.3g (ref32: %.3g), max |alpha - ref64| %.3g"
          % (tag, np.abs(got - score).max(), np.abs(ref32[0] - score).max(), np.abs(rs.alpha.cpu().numpy() - alpha).max()))
    U.assert_close_fp32(got, ref32[0], score, RTOL, ATOL, tag + " score")
    U.assert_close_fp32(rs.alpha.cpu().numpy(), ref32[3], alpha, RTOL, ATOL, tag + " alpha")
    assert (rs.alpha.cpu().numpy()[~live] == 0).all(), tag + ": a dead edge carries attention"


@pytest.mark.parametrize("d,a,act,L,B", CASES)
def test_rescore_against_the_reference_and_the_rebuilt_model(d, a, act, L, B):
    model, data, rows, objs, q_day, rd = _setup(d, a, act, L, B)
    n = len(rows)
    # ---- what explain now sets
    assert rd.n_rel == model.n_rel_true == XR.N_REL and rd.n_time is None and rd.n_hops == L
    assert rd.q_sub.dtype == rd.q_rel.dtype == torch.int64 and rd.q_sub.tolist() == rows[:, 0].tolist() and rd.q_rel.tolist() == rows[:, 1].tolist()
    assert rd.data_row.dtype == rd.time.dtype == rd.q_time.dtype == torch.int32 and rd.q_time.tolist() == q_day.tolist()
    e, day, data_row = (x.cpu().numpy().astype(np.int64) for x in (rd.edges, rd.time, rd.data_row))
    p = state_of(model)
    ref = lambda keep, dt: R.rescore(p, e, day, q_day, rows[:, 0], rows[:, 1], XR.N_ENT, L, act, keep=keep, dtype=dt)
    tag = "d%d a%d %s L%d" % (d, a, act, L)

    # ---- every edge kept: the model's own score
    rs = rd.rescore(model)
    _compare(tag + " keep=None", rs, ref(None, np.float64), ref(None, np.float32))
    assert bool(rs.live.all()) and torch.equal(rs.reached, rd.reached)
    np.testing.assert_allclose(rs.score.cpu().numpy(), rd.score.cpu().numpy(), rtol=2 * RTOL, atol=2 * ATOL)   # two fp32 evaluations
    first = rd.edges[:, 1] == 1
    assert int(first.sum()) > n and torch.equal(rs.alpha[first], rd.alpha[first])           # hop 1: the forward's float, bit for bit
    for keep in (torch.ones(len(e), dtype=torch.uint8, device="cuda"), torch.ones(len(e), dtype=torch.bool, device="cuda"),
                 np.ones(len(e), np.uint8), np.ones(len(e), bool)):
        again = rd.rescore(model, keep=keep)
        assert torch.equal(again.score, rs.score) and torch.equal(again.alpha, rs.alpha) and torch.equal(again.live, rs.live)
    was_training = model.training
    model.train()
    try:
        assert torch.equal(rd.rescore(model).score, rs.score) and model.training             # eval semantics, and the flag comes back
    finally:
        model.train(was_training)

    # ---- the facts deleted, every copy, at every hop
    facts = R.deleted_facts(data, e, data_row, day, rows[:, 0])
    gone = R.rows_of_facts(data, facts)
    m = rd.fact_mask(facts)
    assert m.dtype == torch.bool and np.array_equal(m.cpu().numpy(), R.fact_mask(e, day, data_row, XR.N_REL, facts))
    dup = np.isin(data_row, np.arange(9, 14))
    assert sorted(set(data_row[dup].tolist())) == [9, 10, 11, 12, 13] and m.cpu().numpy()[dup].all()     # all five copies go
    assert torch.equal(rd.data_row_mask(gone), m) and np.array_equal(m.cpu().numpy(), R.data_row_mask(e, data_row, gone))
    some = np.nonzero(m.cpu().numpy())[0][::3]
    assert np.array_equal(rd.data_row_mask(data_row[some], rows=e[some, 0]).cpu().numpy(), R.data_row_mask(e, data_row, data_row[some], e[some, 0]))
    assert np.array_equal(rd.fact_mask(facts, inverse_offset=3).cpu().numpy(), R.fact_mask(e, day, data_row, XR.N_REL, facts, inverse_offset=3))
    keep = ~m
    rs = rd.rescore(model, keep=keep)
    k_h = keep.cpu().numpy()
    assert torch.equal(rd.rescore(model, keep=k_h.astype(np.uint8)).score, rs.score)         # a host array goes along, bits unchanged
    r64, r32 = ref(k_h, np.float64), ref(k_h, np.float32)
    reached = r64[1]
    print("%s: %d facts (%d data rows) deleted, %d of %d edges kept, %d live, %d of %d rows reached" % (tag, len(facts), len(gone), k_h.sum(),
                                                                                                      len(e), r64[2].sum(), reached.sum(), n))
    assert 4 * reached.sum() >= n and (rd.reached.cpu().numpy() & ~reached).any() and (k_h & ~r64[2]).any()
    _compare(tag + " facts deleted", rs, r64, r32)

    # ---- ... is the model's forward on the data without those rows (no deleted row is the last of its day, no day loses its rows)
    cut = R.without_rows(data, gone)
    assert len(cut) == len(data) - len(gone)
    rebuilt = XR.make_model(cut, d, a, act, L)
    rebuilt.load_state_dict(model.state_dict())
    with torch.no_grad():
        fwd = rebuilt(XR.Batch(rows))[0][np.arange(n), objs].cpu().numpy()
    assert np.array_equal(fwd != 0, reached), tag + ": the forward on the rebuilt data reaches other rows"
    U.assert_close_fp32(fwd, r32[0], r64[0], RTOL, ATOL, tag + " forward on the rebuilt data")
    # (two fp32 evaluations of one number, each within the tolerance of it)
    np.testing.assert_allclose(rs.score.cpu().numpy(), fwd, rtol=2 * RTOL, atol=2 * ATOL)
    for m_ in (model, rebuilt):
        for frs in m_._frontiers.pool.values():                     # no frontier is left with a window set
            assert all(getattr(fr, "_window", None) is None for fr in frs)


def test_rescore_refuses_other_models_modes_and_malformed_digraphs():
    from tests import temporal_ref as TR
    model, data, rows, objs, q_day, rd = _setup(*XR.CASES[2])
    with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.*mode must be 'test'"):
        rd.rescore(model, mode="valid")
    with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.*got T_RED_GNN"):
        rd.rescore(TR.make_model(TR.hand_graph(), TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1, TR.HAND_N_TIME, 2, 16, 3, "idd"))
    with pytest.raises(ValueError, match="n_layer=3"):
        rd.rescore(XR.make_model(data, 20, 3, "idd", 3))
    with pytest.raises(ValueError, match="extrapolation.*missing: q_sub"):
        type(rd)(**{**rd.__dict__, "q_sub": None}).rescore(model)
    for col, value, text in ((4, XR.N_ENT, "head or tail out of range"), (3, XR.N_REL + 2, "relation out of range"), (0, None, "not the row of its range")):
        bad = rd.edges.clone()
        bad[0, col] = int(bad[0, 0]) + 1 if value is None else value                          # (None: the row after the edge's own)
        with pytest.raises(ValueError, match=text):
            type(rd)(**{**rd.__dict__, "edges": bad}).rescore(model)
    e = rd.edges.cpu().numpy()
    i = int(np.nonzero((e[1:, 0] == e[:-1, 0]) & (e[1:, 1] == e[:-1, 1]) & (e[1:, 4] > e[:-1, 4]) & (e[1:, 1] == 1))[0][0])
    swapped = rd.edges.clone()
    swapped[i], swapped[i + 1] = rd.edges[i + 1].clone(), rd.edges[i].clone()                # two hop-1 tails of a row change places
    with pytest.raises(ValueError, match=r"ordered by \(row, hop, tail\)"):
        type(rd)(**{**rd.__dict__, "edges": swapped}).rescore(model)
    with pytest.raises(ValueError, match=r"\[F, 4\]"):
        rd.fact_mask([(3, 0, 0)])
    with pytest.raises(ValueError, match="negative"):
        rd.fact_mask([(3, 0, 0, -1)])
    assert torch.equal(rd.rescore(model).reached, rd.reached)       # and the model still scores


def test_fidelity_columns_are_rescores_of_the_path_masks():
    d, a, act, L, B = XR.CASES[1]
    model, data, rows, objs, q_day, _ = _setup(d, a, act, L, B)
    k, n = 3, len(rows)
    batch = XR.Batch(rows)
    f = model.fidelity(batch, objs, k=k)
    rd, paths = f.paths.digraph, f.paths
    assert f.score is rd.score and f.without.shape == f.only.shape == f.reached_without.shape == f.reached_only.shape == (n, k)
    assert torch.equal(f.count, paths.count) and paths.edge.shape[1] == k
    loops = rd.edges[:, 3] == model.n_rel_true
    assert int(loops.sum()) > 0 and bool((rd.data_row[loops] == -1).all())
    for j in range(k):
        m = paths.fact_mask(j + 1)
        assert not bool((m & loops).any())
        wo, on = rd.rescore(model, keep=~m), rd.rescore(model, keep=m | loops)
        assert torch.equal(f.without[:, j], wo.score) and torch.equal(f.reached_without[:, j], wo.reached)
        assert torch.equal(f.only[:, j], on.score) and torch.equal(f.reached_only[:, j], on.reached)
    # the mask of the paths' facts is the reference's, every fact for its own row
    at = paths.edge[:, :k].reshape(-1)
    at = at[at >= 0].cpu().numpy()
    e, day, data_row = (x.cpu().numpy().astype(np.int64) for x in (rd.edges, rd.time, rd.data_row))
    want = R.fact_mask(e, day, data_row, XR.N_REL, np.column_stack([e[at, 2:5], day[at]]), rows=e[at, 0])
    assert np.array_equal(paths.fact_mask(k).cpu().numpy(), want)
    assert torch.equal(f.necessity(), f.score[:, None] - f.without) and torch.equal(f.sufficiency_gap(), f.score[:, None] - f.only)
    assert len(f.format()) == n
    count = f.count.cpu().numpy()
    rw = f.reached_without.cpu().numpy()
    print("paths per row %s; reached without the best j paths: %s of %d" % (count.tolist(), rw.sum(0).tolist(), n))
    # for j past count a row repeats its value at j = count
    for b in range(n):
        for j in range(max(count[b], 1), k):
            assert f.without[b, j] == f.without[b, max(count[b] - 1, 0)] and f.only[b, j] == f.only[b, max(count[b] - 1, 0)]
    # a row whose digraph has at most k paths: those paths' facts and the self-loops are the whole digraph, ``only`` is the score
    total = rd.top_paths(k + 1).count.cpu().numpy()
    few = np.nonzero((total <= k) & (total >= 1))[0]
    assert len(few) >= 1 and (count[few] == total[few]).all()
    p = state_of(model)
    s64 = R.rescore(p, e, day, q_day, rows[:, 0], rows[:, 1], XR.N_ENT, L, act)[0]
    s32 = R.rescore(p, e, day, q_day, rows[:, 0], rows[:, 1], XR.N_ENT, L, act, dtype=np.float32)[0]
    only_at_count = f.only.cpu().numpy()[few, count[few] - 1]
    U.assert_close_fp32(only_at_count, s32[few], s64[few], RTOL, ATOL, "only at j = count")
    np.testing.assert_allclose(only_at_count, f.score.cpu().numpy()[few], rtol=2 * RTOL, atol=2 * ATOL)
    assert f.reached_only.cpu().numpy()[few, count[few] - 1].all()
    # objs=None: each row's own top forecast
    top = model.predict(batch, k=1).ids[:, 0]
    g, h = model.fidelity(batch, k=1), model.fidelity(batch, top.cpu().numpy(), k=1)
    assert torch.equal(g.paths.digraph.edges, h.paths.digraph.edges) and torch.equal(g.without, h.without) and torch.equal(g.only, h.only)
    assert torch.equal(g.paths.digraph.edges[g.paths.digraph.offsets[1:] - 1, 4].long(), top)
    for frs in model._frontiers.pool.values():
        assert all(getattr(fr, "_window", None) is None for fr in frs)


def test_fidelity_all_is_independent_of_the_batching():
    d, a, act, L, B = XR.CASES[2]
    model, data, _, _, _, _ = _setup(d, a, act, L, B)
    pick = data[np.sort(np.random.default_rng(3).choice(np.arange(3000, len(data)), 40, replace=False))]
    out = model.fidelity_all(pick, k=2, batch_size=16)
    assert out["n"] == 40 and out["k"] == 2
    for key in ("necessity_mean", "necessity_median", "sufficiency_gap_mean", "sufficiency_gap_median", "disconnected"):
        assert len(out[key]) == 2 and all(np.isfinite(v) for v in out[key]), key
    assert all(0.0 <= v <= 1.0 for v in out["disconnected"]) and out["disconnected"][0] <= out["disconnected"][1]
    one = model.fidelity_all(torch.as_tensor(pick), k=2, batch_size=40)
    assert one["disconnected"] == out["disconnected"]
    for key in ("necessity_mean", "sufficiency_gap_mean"):
        np.testing.assert_allclose(one[key], out[key], rtol=0, atol=1e-5)
