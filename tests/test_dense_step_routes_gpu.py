"""models._DenseStep forward and backward through every route of its backward, all returned gradients against the fp64 reference.

Each case of dense_ref.ROUTE_CASES (``why`` cites the line of models.py it selects) runs models._DenseStep.apply on dense_ref-style
inputs, reads the x / ws (/ hidden) the step SAVED - exactly what its backward consumed - and checks ALL gradients the backward
returns (agg, hidden_prev, W_h, w_ih, w_hh, b_ih, b_hh and, with a projection, Ws_next) against dense_ref.backward evaluated in fp64
on those saved tensors.  Every element must satisfy

    |gpu - ref64| <= C * (n + n0) * u * S + 1e-30               (dense_ref's docstring defines S, n, n0)

with C = dense_ref.C_BOUND for the two row gradients and C = dense_ref.C_BOUND_WGRAD = 4 x REF32_WORST_RATIO_WGRAD for the weight and
bias gradients, whose n carries the longest chain of rg_gram_tn's summation shape (tests/gram_ref.py), not the row count: a block
order swapped in torch.cat([g_rz, g_n]) or one dropped tail row fails (tests/test_dense_ref.py shows both on the CPU).  The engine
entries are counted, so that a case is known to have taken the route its ``why`` names.  tall_linear's backward (the temporal models
and attn_dim > 16) is held to gram_ref's own bound.  The worst ratios are printed per case (run with -s) and summarised in
ROUTE_RATIOS below, for information only.

What the cases caught: bwd_d16 / bwd_d36 / bwd_d64 (prev_idx given, every entry -1, a previous frontier of 0 rows) failed in the
FORWARD with "prev_idx given without hidden_prev" - an empty hidden_prev has no address.  models._DenseStep.forward now hands the
kernel prev_idx = NULL when there is no row to gather.  The backward itself was found right on every route.

The step is run as the model's forward runs it (models.py:519): engine.prefer_blas(n) first, which selects rocBLAS below 2^17 rows.
Without that call torch's default GEMM library (hipBLASLt) forms the products of the routes below 32768 rows, and it adds the 8192
rows of sums_n8192 / aten_n8191 in far longer chains than rg_gram_tn's shape: grad_w_hh of sums_n8192 measured 0.00229 and grad_w_ih of
aten_n8191 0.00207 against the 0.002 allowed (one element of 3072 each beyond the bound), where rocBLAS measures 0.00045 and
rg_gram_tn on the same operands less.  The library choice is part of the route.
"""
import collections
import types

import numpy as np
import pytest
import torch

from tests import dense_ref as dr
from tests import gram_ref as gr

pytestmark = pytest.mark.gpu

# worst |gpu - ref64| / ((n + n0) u S) per gradient over ROUTE_CASES, as measured on an MI355X (information only)
ROUTE_RATIOS = {"agg": 0.0064, "hidden_prev": 0.015, "W_h": 1.7e-05, "w_ih": 0.00045, "w_hh": 0.00042, "b_ih": 9.7e-05, "b_hh": 9.7e-05,
                "Ws_next": 0.00039, "tall_linear weight": 0.00046, "tall_linear bias": 0.00024, "tall_linear input": 0.5}
# (w_ih: sums_n8192, w_hh: aten_n8191 - the rocBLAS routes; through rg_gram_tn the worst is bwd2_d28's w_ih, 0.00024)
# wall time of this file on an MI355X: 10 s (29 tests)


def _dev(a, dtype=torch.float32, grad=False):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a)).to(dtype).cuda()
    return t.requires_grad_() if grad else t


def _check(what, gpu, ref, S, n, c):
    gpu = gpu.detach().cpu().numpy().astype(np.float64)
    assert gpu.shape == np.shape(ref), "%s: shape %s, expected %s" % (what, gpu.shape, np.shape(ref))
    assert not np.isnan(gpu).any(), "%s: %d NaN" % (what, int(np.isnan(gpu).sum()))
    ok = np.abs(gpu - ref) <= dr.bound(S, n, dr.N0_STEP, c)
    ratio = dr.worst_ratio(gpu, ref, S, n, dr.N0_STEP)
    assert ok.all(), ("%s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g); first at %s: gpu %.9g ref %.9g"
                      % (what, int((~ok).sum()), ok.size, ratio, c, np.argwhere(~ok)[0], gpu[~ok][0], np.asarray(ref)[~ok][0]))
    return ratio


def _expected_calls(case):
    """How often the backward reaches each engine entry (models.py:160-204)."""
    tall, fused = case.n >= 32768, case.d <= 64 and case.n >= 8192
    bwd2 = fused and tall and case.prev != "none"
    exp = dict(dense_train_bwd2=int(bwd2), dense_train_bwd=int(fused and not bwd2), rows_addmm=int(bool(case.attn_dim) and tall))
    exp["gram_tn"] = (4 if bwd2 else 3 if tall else 0) + int(bool(case.attn_dim) and tall)
    return exp


@pytest.mark.parametrize("name", list(dr.ROUTE_CASES))
def test_dense_step_gradients_vs_reference(name, monkeypatch):
    from red_gnn_amd import engine, models
    case = dr.ROUTE_CASES[name]
    x = dr.inputs(case)
    n, d, n_old = case.n, case.d, x["n_old"]
    act = {v: k for k, v in dr.ACT.items()}[case.act]
    leaf = {k: _dev(x[k], grad=True) for k in ("agg", "W_h", "w_ih", "w_hh", "b_ih", "b_hh")}
    leaf["hidden_prev"] = _dev(x["hidden_prev"][:n_old], grad=True)
    if case.attn_dim:
        leaf["Ws_next"] = _dev(x["Ws_next"], grad=True)
    p = x["prev_idx"]
    new_of_old = np.empty(n_old, np.int64)
    new_of_old[p[p >= 0]] = np.nonzero(p >= 0)[0]
    gate = types.SimpleNamespace(weight_ih_l0=leaf["w_ih"], weight_hh_l0=leaf["w_hh"], bias_ih_l0=leaf["b_ih"], bias_hh_l0=leaf["b_hh"])
    calls = collections.Counter()
    for entry in ("dense_train_bwd2", "dense_train_bwd", "gram_tn", "rows_addmm"):
        def counted(*a, _f=getattr(engine, entry), _k=entry, **kw):
            calls[_k] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(engine, entry, counted)
    engine.prefer_blas(n)      # models.py:519: the forward picks the GEMM library by the row count before every step
    out = models._DenseStep.apply(leaf["agg"], leaf["hidden_prev"], leaf["W_h"], leaf["w_ih"], leaf["w_hh"], leaf["b_ih"], leaf["b_hh"],
                                  leaf.get("Ws_next"), _dev(p, torch.int32), _dev(new_of_old, torch.int32), _dev(x["mask"]), act, gate, case.keep)
    hidden, a_s = out if case.attn_dim else (out, None)
    saved = hidden.grad_fn.saved_tensors      # agg, x, ws, W_h, w_ih, w_hh, old_new, mask, Ws_next, hidden
    xs, ws, hs = (t.detach().cpu().numpy() for t in (saved[1], saved[2], saved[9]))
    hs = hs if case.attn_dim else None
    assert xs.shape == (n, d) and ws.shape == (n, 5 * d) and (hs is None or np.array_equal(hs, hidden.detach().cpu().numpy()))
    outs, gouts = [hidden], [_dev(x["grad_hidden"])]
    if case.attn_dim:
        outs, gouts = outs + [a_s], gouts + [_dev(x["g_as"])]
    names = list(leaf)
    grads = dict(zip(names, torch.autograd.grad(outs, [leaf[k] for k in names], gouts)))
    torch.cuda.synchronize()
    assert dict(calls) == {k: v for k, v in _expected_calls(case).items() if v}, (name, dict(calls))

    b = dr.route_backward(case, x, xs, ws, hs)
    pairs = [("agg", "dagg", dr.C_BOUND), ("hidden_prev", "grad_prev", dr.C_BOUND), ("W_h", "grad_W_h", dr.C_BOUND_WGRAD),
             ("w_ih", "grad_w_ih", dr.C_BOUND_WGRAD), ("w_hh", "grad_w_hh", dr.C_BOUND_WGRAD), ("b_ih", "grad_b_ih", dr.C_BOUND_WGRAD),
             ("b_hh", "grad_b_hh", dr.C_BOUND_WGRAD)] + ([("Ws_next", "grad_Ws", dr.C_BOUND_WGRAD)] if case.attn_dim else [])
    ratios = {o: _check("%s grad of %s" % (name, k), grads[k], getattr(b, o), b.S[o], b.n[o], c) for k, o, c in pairs}
    print("%s: %s" % (name, " ".join("%s=%.3g" % kv for kv in ratios.items())))


@pytest.mark.parametrize("m,n", [(1, 64), (32, 64), (384, 128)])
def test_tall_linear_backward_vs_reference(m, n, monkeypatch):
    """models.tall_linear with a bias at 32768 rows (models.py:91 _gram_tn -> models.py:68 engine.gram_tn; [384, 128] tiled): the weight
    gradient within gram_ref's bound of fp64, the bias gradient (models.py:92, g.sum(0)) within the column sum's, the input gradient
    (models.py:90) within the row-wise products' bound."""
    from red_gnn_amd import engine, models
    rows = 32768
    case = gr._case("normal", "normal", m, n, rows, "models.py:91", seed=7000 + m)
    x = gr.inputs(case)
    rng = np.random.default_rng(7100 + m)
    w_np, b_np = (rng.standard_normal((m, n)) * n ** -0.5).astype(np.float32), rng.standard_normal(m).astype(np.float32)
    xin, w, bias, g = _dev(x["x"], grad=True), _dev(w_np, grad=True), _dev(b_np, grad=True), _dev(x["g"])
    calls = []
    monkeypatch.setattr(engine, "gram_tn", lambda *a, _f=engine.gram_tn, **kw: (calls.append(1), _f(*a, **kw))[1])
    engine.prefer_blas(rows)
    y = models.tall_linear(xin, w, bias)
    gx, gw, gb = torch.autograd.grad(y, (xin, w, bias), g)
    torch.cuda.synchronize()
    assert len(calls) == 1
    ref = gr.gram(x["g"], x["x"])
    ok_w, ok_b = gr.agrees(case, gw.cpu().numpy(), gb.cpu().numpy(), ref)
    r_w = gr.worst_ratio(gw.cpu().numpy(), ref.out, ref.S["out"], ref.n["out"], gr.N0_GRAM)
    r_b = gr.worst_ratio(gb.cpu().numpy(), ref.colsum, ref.S["colsum"], ref.n["colsum"], gr.N0_COLSUM)
    g64, w64 = x["g"].astype(np.float64), w_np.astype(np.float64)
    S_x = np.abs(g64) @ np.abs(w64)
    r_x = dr.worst_ratio(gx.cpu().numpy(), g64 @ w64, S_x, m, dr.N0_ROWS)
    print("tall_linear %dx%d: weight=%.3g bias=%.3g (allowed %.3g) input=%.3g (allowed %.3g)" % (m, n, r_w, r_b, gr.C_BOUND_GRAM, r_x, dr.C_BOUND_ROWS))
    assert gw.shape == (m, n) and gb.shape == (m,) and not torch.isnan(gw).any() and not torch.isnan(gb).any()
    assert ok_w and ok_b, (r_w, r_b, gr.C_BOUND_GRAM)
    assert (np.abs(gx.cpu().numpy() - g64 @ w64) <= dr.bound(S_x, m, dr.N0_ROWS, dr.C_BOUND_ROWS)).all(), r_x
