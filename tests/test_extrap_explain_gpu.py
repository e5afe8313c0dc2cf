"""extrapolation.T_RED_GNN.explain on the GPU: the r-digraph of a forecast (s, p, t, o) with the attention, the data row and the day of
every edge, against the float64 walk of tests/extrap_ref.py, and its properties.  Tolerances: alpha as tests/test_explain_gpu.py
(rtol 1e-4 / atol 1e-5), logits as the extrapolation parity tests (rtol 1e-4 / atol 5e-5); integers exact."""
import functools

import numpy as np
import pytest
import torch

from tests import explain_ref as XR
from tests import extrap_ref as R
from tests.test_temporal_explain_gpu import _rows

pytestmark = pytest.mark.gpu

RTOL, ATOL, ATOL_H = 1e-4, 1e-5, 5e-5
FIELDS = ("edges", "alpha", "time", "offsets", "reached", "score", "q_time", "data_row")


@functools.lru_cache(maxsize=None)
def _setup(d, a, act, n_layer, B):
    """Model, data, queries, the float64 walk and the rows (query, answer): answers inside and outside the last level."""
    from red_gnn_amd import extrapolation as X
    from tests.temporal_ref import state_of
    data, q = R.make_case(d, B)
    model = R.make_model(data, d, a, act, n_layer)
    off = X.get_time_offset_list(data, 24)
    walk = R.walk(state_of(model), data, off, 24, R.N_ENT, R.N_REL, q[:, 0], q[:, 1], q[:, 3], n_layer, act)
    q_of, objs = _rows(walk[1], B, R.N_ENT, np.random.default_rng(0), per_query=2 if B > 9 else 3)
    return model, data, q, off, walk, q_of, objs


@pytest.mark.parametrize("d,a,act,n_layer,B", R.CASES + [(32, 30, "relu", 4, 5)])
def test_explain_vs_walk(d, a, act, n_layer, B):
    model, data, q, off, (logits, last, hops, cur_t), q_of, objs = _setup(d, a, act, n_layer, B)
    n_data = len(data)
    batch = R.Batch(q[q_of])
    rd = model.explain(batch, objs)
    edges, data_row, day, alpha, offsets, reached = R.expected_digraph(hops, q_of, objs, last, 0.0, R.N_ENT, n_data, model.graph)
    assert reached.any() and not reached.all()
    got = rd.edges.cpu().numpy()
    assert rd.edges.dtype == torch.int32 and got.shape == edges.shape and np.array_equal(got, edges)
    assert rd.data_row.dtype == torch.int32 and np.array_equal(rd.data_row.cpu().numpy(), data_row)
    assert rd.time.dtype == torch.int32 and np.array_equal(rd.time.cpu().numpy(), day)
    assert rd.q_time.dtype == torch.int32 and np.array_equal(rd.q_time.cpu().numpy(), cur_t[q_of])
    assert np.array_equal(rd.offsets.cpu().numpy(), offsets) and np.array_equal(rd.reached.cpu().numpy(), reached)
    assert rd.n_hops == n_layer
    np.testing.assert_allclose(rd.alpha.cpu().numpy(), alpha, rtol=RTOL, atol=ATOL)
    lag = rd.lag()
    assert lag.dtype == torch.int32 and np.array_equal(lag.cpu().numpy(), cur_t[q_of][edges[:, 0]] - day)
    # score: the logit of o, 0 where it was not reached
    key = last[:, 0] * R.N_ENT + last[:, 1]
    want = np.array([logits[np.searchsorted(key, qq * R.N_ENT + o)] if r else 0.0 for qq, o, r in zip(q_of, objs, reached)])
    np.testing.assert_allclose(rd.score.cpu().numpy(), want, rtol=RTOL, atol=ATOL_H)
    assert (rd.score.cpu().numpy()[~reached] == 0).all()
    # every kept data row lies in its row's window, or is a self-loop (relation id n_rel, head == tail)
    lo, hi = off[np.maximum(cur_t - R.WINDOW, 0)][q_of], off[cur_t][q_of]
    loop = data_row < 0
    assert loop.any() and (~loop).any()
    assert ((data_row[~loop] >= lo[got[~loop, 0]]) & (data_row[~loop] < hi[got[~loop, 0]])).all()
    assert (got[loop, 3] == R.N_REL).all() and (got[loop, 2] == got[loop, 4]).all() and (data_row[loop] == -1).all()
    assert np.array_equal(data[data_row[~loop], :3], got[~loop][:, 2:5])
    # tau > 0 on the device's own tau = 0 alphas: same edges, same order, bitwise alphas
    e0, a0, r0 = got, rd.alpha.cpu().numpy(), rd.data_row.cpu().numpy()
    for tau in (0.3, 0.6):
        ok = XR.rdigraph_mask(e0[:, 0], e0[:, 1], e0[:, 2], e0[:, 4], a0, objs, reached, tau, R.N_ENT, n_layer)
        rd_t = model.explain(batch, objs, min_alpha=tau)
        assert np.array_equal(rd_t.edges.cpu().numpy(), e0[ok]) and np.array_equal(rd_t.data_row.cpu().numpy(), r0[ok]), tau
        assert np.array_equal(rd_t.alpha.cpu().numpy(), a0[ok]) and (rd_t.alpha.cpu().numpy() >= tau).all(), tau
        assert np.array_equal(rd_t.offsets.cpu().numpy()[1:], np.cumsum(np.bincount(e0[ok][:, 0], minlength=len(q_of))))
    # strongest_paths works unchanged: a path from s to o for every reached row
    rl, en, pr = (x.cpu().numpy() for x in rd.strongest_paths())
    assert (en[reached, 0] == q[q_of][reached, 0]).all() and (en[reached, -1] == objs[reached]).all() and (pr[reached] > 0).all()
    assert (en[~reached] == -1).all()


def test_duplicated_rows_and_an_empty_window():
    """The equal data rows 9..13 are separate edges with equal alpha; a query on the first day has an empty window and its digraph
    holds self-loops only."""
    d, a, act, n_layer, B = R.CASES[1]
    model, data, q, off, _, _, _ = _setup(d, a, act, n_layer, B)
    s, p, o, t = data[9]
    later = np.array([[s, p, o, t + 24 * 5], [s, 0, s, data[0, 3]]])
    assert off[data[0, 3] // 24] == 0                            # no row before the first day
    rd = model.explain(R.Batch(later), [o, s])
    e, row, off_e = rd.edges.cpu().numpy(), rd.data_row.cpu().numpy(), rd.offsets.cpu().numpy()
    assert rd.reached.all()
    m = (e[:, 0] == 0) & (e[:, 1] == 1) & np.isin(row, np.arange(9, 14))
    assert sorted(row[m].tolist()) == [9, 10, 11, 12, 13] and len(set(rd.alpha.cpu().numpy()[m].tolist())) == 1
    assert (e[m, 2:5] == [s, p, o]).all()
    mine = slice(off_e[1], off_e[2])
    assert off_e[2] - off_e[1] == n_layer and (row[mine] == -1).all() and (e[mine, 2:5] == [s, R.N_REL, s]).all()
    assert (rd.lag().cpu().numpy()[mine] == data[0, 3] // 24).all()      # the self-loops carry the window's first day, day 0


def test_top_answer_determinism_batch_invariance_flags_and_errors():
    d, a, act, n_layer, B = R.CASES[0]
    model, data, q, off, walk, q_of, objs = _setup(d, a, act, n_layer, B)
    batch = R.Batch(q)
    with torch.no_grad():
        before = model(batch)[0].clone()
    top = model.predict(batch, k=1)
    rd_top = model.explain(batch)
    rd_arg = model.explain(batch, top.ids[:, 0].cpu().numpy())
    for f in FIELDS:
        assert torch.equal(getattr(rd_top, f), getattr(rd_arg, f)), f
    assert rd_top.reached.all() and torch.equal(rd_top.score, top.scores[:, 0])
    assert torch.equal(rd_top.edges[rd_top.offsets[1:] - 1, 4].long(), top.ids[:, 0])       # every row's last edge ends at its answer
    rows = R.Batch(q[q_of])
    rd, rd2 = model.explain(rows, objs), model.explain(rows, objs)
    for f in FIELDS:
        assert torch.equal(getattr(rd, f), getattr(rd2, f)), f
    off_e = rd.offsets.cpu().numpy()
    for b in range(0, len(q_of), 5):
        one = model.explain(R.Batch(q[q_of][b:b + 1]), objs[b:b + 1])
        sl = slice(off_e[b], off_e[b + 1])
        e = rd.edges[sl].clone()
        e[:, 0] = 0
        assert torch.equal(one.edges, e) and torch.equal(one.data_row, rd.data_row[sl]) and torch.equal(one.time, rd.time[sl]), b
        # (the forward's dense products choose their tiling by the number of rows: the attention inputs of a row may differ in the
        # last bits between a batch of one and the whole batch)
        np.testing.assert_allclose(one.alpha.cpu().numpy(), rd.alpha[sl].cpu().numpy(), rtol=RTOL, atol=ATOL)
    model.train()
    model.time_embed.eval()
    flags = [m.training for m in model.modules()]
    rd3 = model.explain(rows, objs)
    assert [m.training for m in model.modules()] == flags
    model.eval()
    for f in FIELDS:
        assert torch.equal(getattr(rd, f), getattr(rd3, f)), f
    with pytest.raises(ValueError):
        model.explain(rows, np.full(len(objs), R.N_ENT))
    with pytest.raises(ValueError):
        model.explain(rows, objs[:-1])
    for frs in model._frontiers.pool.values():                   # no frontier window is left set
        assert all(getattr(fr, "_window", None) is None for fr in frs)
    with torch.no_grad():
        assert torch.equal(model(batch)[0], before)


def test_a_failure_inside_the_walk_leaves_no_windowed_frontier(monkeypatch):
    from red_gnn_amd import engine
    d, a, act, n_layer, B = R.CASES[2]
    model, data, q, off, walk, q_of, objs = _setup(d, a, act, n_layer, B)
    with torch.no_grad():
        before = model(R.Batch(q))[0].clone()

    def boom(*args, **kw):
        raise RuntimeError("boom")
    monkeypatch.setattr(engine, "xexplain_hop", boom)
    with pytest.raises(RuntimeError):
        model.explain(R.Batch(q))
    monkeypatch.undo()
    for frs in model._frontiers.pool.values():
        assert all(getattr(fr, "_window", None) is None for fr in frs)
    with torch.no_grad():
        assert torch.equal(model(R.Batch(q))[0], before)
    assert model.explain(R.Batch(q)).reached.all()


def test_entry_points_require_a_windowed_frontier():
    import ctypes as C
    from red_gnn_amd import _lib, engine
    d, a, act, n_layer, B = R.CASES[2]
    model = _setup(d, a, act, n_layer, B)[0]
    L, s = _lib.lib(), _lib.stream_ptr()
    fr = engine.Frontier(R.N_ENT, 2, 3)
    fr.reset(torch.zeros(2, dtype=torch.int32, device="cuda"))
    fr.expand(model.graph)
    W = (R.N_ENT + 31) // 32
    marks = torch.zeros((2, W), dtype=torch.int32, device="cuda")
    prev, wp = torch.zeros_like(marks), torch.zeros(marks.numel() + 1, dtype=torch.int32, device="cuda")
    f32 = torch.zeros((R.N_REL + 2, 4), dtype=torch.float32, device="cuda")
    scr = torch.zeros(L.rg_explain_scratch_bytes(fr.handle) + 512, dtype=torch.uint8, device="cuda")
    scr_p = (scr.data_ptr() + 255) // 256 * 256
    n_e = C.c_int64()
    p = _lib.ptr
    rc = L.rg_xexplain_count(fr.handle, model.graph.handle, 2, R.N_ENT, 1, p(marks), p(f32), p(f32), p(f32), 4, p(f32), p(f32), 3, 0.0,
                             p(prev), p(wp), C.c_void_p(scr_p), scr.numel() - (scr_p - scr.data_ptr()), C.byref(n_e), s)
    assert rc != 0 and b"rg_frontier_set_window" in L.rg_last_error()
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    fr.set_window(z, z + 5, len(model.row_time))
    rc = L.rg_xexplain_count(fr.handle, model.graph.handle, 2, R.N_ENT, 1, p(marks), p(f32), p(f32), p(f32), 4, p(f32), p(f32), 3, 0.0,
                             p(prev), p(wp), C.c_void_p(scr_p), scr.numel() - (scr_p - scr.data_ptr()), C.byref(n_e), s)
    assert rc == 0 and n_e.value == 0                            # (no marks: no edges)
    torch.cuda.synchronize()
