"""extrapolation.T_RED_GNN.predict on the GPU: the forecasts against numpy's selection over the logits and node set of the model's own
forward (bit for bit), the softmax against float64, consistency with rank_batch, and the properties of the call.  The graph and the
parametrisation are those of test_gpu_parity.test_temporal_extrapolation_training_step_vs_oracle_autograd (tests/extrap_ref.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import extrap_ref as R

pytestmark = pytest.mark.gpu

K = 10


@functools.lru_cache(maxsize=None)
def _setup(d, a, act, n_layer, B):
    from red_gnn_amd import extrapolation as X
    data, q = R.make_case(d, B)
    model = R.make_model(data, d, a, act, n_layer)
    return X, model, data, q, X.known_objects_index(data, R.N_REL, False), X.known_objects_index(data, R.N_REL, True)


def _forward(model, q):
    with torch.no_grad():
        logits, soft, nodes, _ = model._run(R.Batch(q), dense=False)
    nodes = nodes.cpu().numpy().astype(np.int64)
    seg_ptr = np.searchsorted(nodes[:, 0], np.arange(len(q) + 1))
    return logits.cpu().numpy(), soft.cpu().numpy(), nodes, seg_ptr


@pytest.mark.parametrize("d,a,act,n_layer,B", R.CASES)
def test_predict_equals_numpy_selection_over_the_forward(d, a, act, n_layer, B):
    X, model, data, q, sp, spt = _setup(d, a, act, n_layer, B)
    logits, _, nodes, seg_ptr = _forward(model, q)
    sizes = np.diff(seg_ptr)
    short = 0
    for index in (None, sp, spt):
        pred = model.predict(R.Batch(q), k=K, known=index)
        assert pred.ids.dtype == torch.int64 and pred.scores.dtype == pred.prob.dtype == torch.float32
        assert pred.ids.is_cuda and pred.ids.shape == pred.scores.shape == pred.prob.shape == (B, K) and not pred.scores.requires_grad
        q_key = None if index is None else index.query_keys(q[:, 0], q[:, 1], q[:, 3])
        ids, val, prob = R.segment_topk_ref(logits, nodes[:, 1], seg_ptr, K, q_key, None if index is None else tuple(index))
        assert np.array_equal(pred.ids.cpu().numpy(), ids)
        assert pred.scores.cpu().numpy().tobytes() == val.tobytes()
        np.testing.assert_allclose(pred.prob.cpu().numpy(), prob, rtol=2e-4, atol=1e-7)
        n_kept = (ids >= 0).sum(1)
        short += int((n_kept < K).sum())
        assert ((ids >= 0) == (np.arange(K) < n_kept[:, None])).all()               # -1 only past the end
        if index is None:
            assert np.array_equal(n_kept, np.minimum(sizes, K))
        if index is sp:
            hidden = np.array([np.isin(nodes[seg_ptr[b]:seg_ptr[b + 1], 1], sp.objects(q[b, 0], q[b, 1])).sum() for b in range(B)])
            assert hidden.max() > 0 and np.array_equal(n_kept, np.minimum(sizes - hidden, K))
            for b in range(B):
                assert not np.isin(ids[b][ids[b] >= 0], sp.objects(q[b, 0], q[b, 1])).any()
    print("segments of %d..%d pairs; %d rows shorter than k" % (sizes.min(), sizes.max(), short))
    assert len(model._known_dev) == 2                                               # each index went to the device once


@pytest.mark.parametrize("d,a,act,n_layer,B", R.CASES)
def test_predict_agrees_with_rank_batch(d, a, act, n_layer, B):
    """rank_fil of the j-th forecast is j + 1 wherever its softmax value differs from every other kept entity's of its row (rank_batch
    ranks by the float32 softmax, in which distinct logits can tie); such ties may cost at most 10 % of the returned positions."""
    X, model, data, q, sp, spt = _setup(d, a, act, n_layer, B)
    pred = model.predict(R.Batch(q), k=K, known=sp)
    ids = pred.ids.cpu().numpy()
    _, soft, nodes, seg_ptr = _forward(model, q)
    checked = skipped = 0
    for j in range(K):
        rows = np.flatnonzero(ids[:, j] >= 0)
        if len(rows) == 0:
            continue
        rb = model.rank_batch(R.Batch(q[rows]), ids[rows, j], sp)
        soft_j, nodes_j = rb.soft.cpu().numpy(), rb.nodes.cpu().numpy()
        rank_fil = rb.rank_fil.cpu().numpy()
        assert rb.found.all()
        for i, b in enumerate(rows):
            seg = nodes_j[:, 0] == i
            e, s = nodes_j[seg, 1], soft_j[seg]
            kept = ~np.isin(e, np.setdiff1d(sp.objects(q[b, 0], q[b, 1]), [ids[b, j]]))
            mine = s[e == ids[b, j]][0]
            if (s[kept] == mine).sum() > 1:
                skipped += 1
                continue
            checked += 1
            assert rank_fil[i] == j + 1, (b, j, rank_fil[i])
    print("%d positions checked, %d skipped for softmax ties" % (checked, skipped))
    assert checked > 0 and skipped <= 0.1 * (checked + skipped)


def test_batch_split_training_flags_and_window():
    d, a, act, n_layer, B = R.CASES[1]
    X, model, data, q, sp, spt = _setup(d, a, act, n_layer, B)
    with torch.no_grad():
        before = model(R.Batch(q))[0].clone()
    whole = model.predict(R.Batch(q), k=K + 1, known=spt)
    lo, hi = model.predict(R.Batch(q[:7]), k=K + 1, known=spt), model.predict(R.Batch(q[7:]), k=K + 1, known=spt)
    # The forward's dense products choose their tiling by the number of rows, so a query's logits may differ in the last bits between
    # two splits of the batch (the selection itself is bitwise split-invariant: test_segment_topk_gpu).  What must hold: the logits
    # agree at the logit tolerance, and every position whose logit is further than twice that from both neighbours holds the same id.
    ws, ps = whole.scores.cpu().numpy(), torch.cat([lo.scores, hi.scores]).cpu().numpy()
    wi, pi = whole.ids.cpu().numpy(), torch.cat([lo.ids, hi.ids]).cpu().numpy()
    assert np.array_equal(wi >= 0, pi >= 0)
    np.testing.assert_allclose(ps, ws, rtol=1e-4, atol=5e-5)
    margin = 2 * (5e-5 + 1e-4 * np.abs(ws[:, :K]))
    with np.errstate(invalid="ignore"):                          # (-inf - -inf past the end of a short row)
        gap = np.nan_to_num(ws[:, :K] - ws[:, 1:K + 1], nan=np.inf)
    above = np.concatenate([np.full((B, 1), np.inf), gap[:, :K - 1]], 1)
    clear = (wi[:, :K] >= 0) & (above > margin) & (gap > margin)
    assert clear.mean() > 0.5 and np.array_equal(wi[:, :K][clear], pi[:, :K][clear])
    whole = model.predict(R.Batch(q), k=K, known=spt)
    again = model.predict(R.Batch(q), k=K, known=spt)
    assert all(torch.equal(getattr(whole, f), getattr(again, f)) for f in ("ids", "scores", "prob"))
    model.train()
    model.time_embed.eval()
    flags = [m.training for m in model.modules()]
    assert True in flags and False in flags
    trained = model.predict(R.Batch(q), k=K, known=spt)
    assert [m.training for m in model.modules()] == flags
    model.eval()
    assert torch.equal(trained.ids, whole.ids) and torch.equal(trained.scores, whole.scores)
    for frs in model._frontiers.pool.values():                   # no frontier window is left set
        assert all(getattr(fr, "_window", None) is None for fr in frs)
    with torch.no_grad():
        assert torch.equal(model(R.Batch(q))[0], before)
    one = model.predict(R.Batch(q), k=1)
    top = model.predict(R.Batch(q), k=1024)
    assert torch.equal(one.ids[:, 0], top.ids[:, 0]) and (top.ids[:, R.N_ENT:] == -1).all() and torch.isinf(top.scores[:, R.N_ENT:]).all()
