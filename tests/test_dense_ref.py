"""The dense-step reference (tests/dense_ref.py) checked on the CPU: by hand, against torch.gru_cell and torch autograd in fp64, its own
fp32 evaluation against the bound the GPU tests use (so the bound is known to be satisfiable by a correct fp32 implementation before a
GPU is involved), and the bound against three deliberately wrong copies of the operation (so it is known to reject a subtly wrong
kernel)."""
import functools
import math
import types

import numpy as np
import pytest
import torch

from tests import dense_ref as dr


def test_dense_ref_on_one_row_by_hand():
    """d = 1, one row, identity activation, no mask:  agg = 2, W_h = 1/2, h0 = 1/4, g = 1
        pre = x = 1
        r = sigmoid(ln 3 * 1) = 3/4          (W_ir = ln 3, W_hr = 0, no bias)
        z = sigmoid(0) = 1/2                 (W_iz = W_hz = 0)
        hn = 2 * 1/4 + 1 = 3/2               (W_hn = 2, b_hn = 1)
        n = tanh(-3/2 + 3/8 + atanh(1/2) + 3/4 * 3/2) = tanh(atanh(1/2)) = 1/2       (W_in = -3/2, b_in = 3/8 + atanh 1/2)
        hidden = 1/2 * 1/2 + 1/2 * 1/4 = 3/8;   a_s = 4 * 3/8 = 3/2 (Ws = 4), padded to 4 columns
        S_pre = S_x = 1;  S_r = r (1 - r) (ln 3 + 1) + r
      backward
        dn = 1 * 1/2 * (1 - 1/4) = 3/8;  dr = 3/8 * 3/2 * 3/16 = 27/256;  dz = (1/4 - 1/2) * 1/4 = -1/16;  dn r = 9/32
        dx = 27/256 ln 3 - 9/16;  dh0 = 1/2 + 9/32 * 2 = 17/16;  dpre = dx;  dagg = dx / 2"""
    ln3, b_in = math.log(3.0), 0.375 + math.atanh(0.5)
    a = lambda *v: np.array(v, np.float64)
    W_h, w_ih, w_hh = a(0.5).reshape(1, 1), a(ln3, 0.0, -1.5).reshape(3, 1), a(0.0, 0.0, 2.0).reshape(3, 1)
    f = dr.forward(a(2.0).reshape(1, 1), a(0.25).reshape(1, 1), np.array([0], np.int32), W_h, 0, w_ih, w_hh, a(0, 0, b_in), a(0, 0, 1.0),
                   None, a(4.0).reshape(1, 1), 4)
    np.testing.assert_allclose(f.x, [[1.0]], rtol=1e-15)
    np.testing.assert_allclose(f.ws.reshape(5), [0.75, 0.5, 0.5, 0.25, 1.5], rtol=1e-14)
    np.testing.assert_allclose(f.hidden, [[0.375]], rtol=1e-14)
    np.testing.assert_allclose(f.a_s, [[1.5, 0, 0, 0]], rtol=1e-14)
    np.testing.assert_allclose(f.S["x"], [[1.0]], rtol=1e-15)
    np.testing.assert_allclose(f.S["ws"][0, 0, 0], 0.1875 * (ln3 + 1) + 0.75, rtol=1e-14)
    assert f.S["a_s"][0, 1:].tolist() == [0, 0, 0] and f.n["a_s"] == 6 and f.n["x"] == 1
    b = dr.backward(a(1.0).reshape(1, 1), f.ws.reshape(1, 5), f.x, None, 1.0, 0, W_h, w_ih, w_hh, np.array([0], np.int32), 1)
    dx = 27 / 256 * ln3 - 9 / 16
    np.testing.assert_allclose(b.dgi, [[27 / 256, -1 / 16, 3 / 8]], rtol=1e-14)
    np.testing.assert_allclose(b.dgh, [[27 / 256, -1 / 16, 9 / 32]], rtol=1e-14)
    np.testing.assert_allclose(b.dgh_n, [[9 / 32]], rtol=1e-14)
    np.testing.assert_allclose(b.dpre, [[dx]], rtol=1e-14)
    np.testing.assert_allclose(b.dagg, [[dx / 2]], rtol=1e-14)
    np.testing.assert_allclose(b.dh0, [[17 / 16]], rtol=1e-14)
    np.testing.assert_allclose(b.grad_prev, [[17 / 16]], rtol=1e-14)
    # S of dz: |g| (|h0| + |n|) |z| (1 + |z|) = 3/4 * 1/2 * 3/2
    np.testing.assert_allclose(b.S["dgi"][0, 1], 0.5625, rtol=1e-14)


def _torch_step(case, x, mask64):
    """The step in torch float64 with every intermediate the kernels emit kept for autograd: index_copy carry, mask, GRU cell."""
    t = lambda a, grad=False: None if a is None else torch.tensor(np.asarray(a, np.float64), requires_grad=grad)
    d, n = case.d, case.n
    agg, W_h, w_ih, w_hh, b_ih, b_hh = (t(x[k], True) for k in ("agg", "W_h", "w_ih", "w_hh", "b_ih", "b_hh"))
    hp = t(x["hidden_prev"], True)
    h0 = torch.zeros(n, d, dtype=torch.float64, requires_grad=True)
    if x["prev_idx"] is not None and x["n_old"]:
        p = np.asarray(x["prev_idx"], np.int64)
        new_of_old = np.empty(x["n_old"], np.int64)
        new_of_old[p[p >= 0]] = np.nonzero(p >= 0)[0]
        h0 = h0.index_copy(0, torch.as_tensor(new_of_old), hp)      # models.py:81
        h0.retain_grad()
    pre = agg @ W_h.T
    pre.retain_grad()
    a = pre if case.act == 0 else torch.relu(pre) if case.act == 1 else torch.tanh(pre)
    xx = a if mask64 is None else a * t(mask64)
    gi, gh = xx @ w_ih.T + b_ih, h0 @ w_hh.T + b_hh
    gi.retain_grad(), gh.retain_grad()
    r, z = torch.sigmoid(gi[:, :d] + gh[:, :d]), torch.sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
    ng = torch.tanh(gi[:, 2 * d:] + r * gh[:, 2 * d:])
    hidden = (1 - z) * ng + z * h0
    cell = torch.gru_cell(xx, h0, w_ih, w_hh, b_ih, b_hh)
    return dict(agg=agg, hp=hp, h0=h0, pre=pre, x=xx, gi=gi, gh=gh, r=r, z=z, ng=ng, hidden=hidden, cell=cell, W_h=W_h, w_ih=w_ih, w_hh=w_hh,
                b_ih=b_ih, b_hh=b_hh)


@pytest.mark.parametrize("name", ["d20_tanh_mask", "d36_relu_mask", "d32_idd", "d48_tanh", "n17", "as5", "n1"])
def test_reference_equals_torch(name):
    """forward == torch.gru_cell around the same W_h / mask / carry in fp64; backward == autograd of that step for every output,
    including dgh[:, :2d] == dgi[:, :2d] and grad_prev == dh0 gathered by prev_idx."""
    case = dr.CASES[name]
    x = dr.inputs(case)
    d = case.d
    # the mask's kept value 1 / keep exactly in fp64, so that x * keep is tanh(pre) as the tanh adjoint assumes; the kernels' keep is a C
    # float, which dr.backward rounds to: pass the fp64 value through a case whose keep is representable
    mask64 = None if x["mask"] is None else (x["mask"] > 0) / 0.75
    case = types.SimpleNamespace(**dict(vars(case), keep=0.75))
    x = dict(x, mask=mask64)
    T = _torch_step(case, x, mask64)
    f = dr.step_forward(case, x)
    tol = dict(rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(T["cell"].detach().numpy(), T["hidden"].detach().numpy(), **tol)
    np.testing.assert_allclose(f.hidden, T["cell"].detach().numpy(), **tol)
    np.testing.assert_allclose(f.x, T["x"].detach().numpy(), **tol)
    b_hn = np.asarray(x["b_hh"], np.float64)[2 * d:]
    for i, k in enumerate(("r", "z", "ng", "h0")):
        np.testing.assert_allclose(f.ws[:, i], T[k].detach().numpy(), err_msg=k, **tol)
    np.testing.assert_allclose(f.ws[:, 4], T["gh"].detach().numpy()[:, 2 * d:], **tol)
    assert np.abs(b_hn).min() > 0      # so a dropped b_hn would show
    if case.attn_dim:
        np.testing.assert_allclose(f.a_s[:, :case.attn_dim], f.hidden @ np.asarray(x["Ws_next"], np.float64).T, **tol)
        assert not f.a_s[:, case.attn_dim:].any()
    T["hidden"].backward(torch.as_tensor(np.asarray(x["grad_hidden"], np.float64)))
    b = dr.step_backward(case, x, f.x, f.ws.reshape(case.n, 5 * d))
    g = lambda k: T[k].grad.numpy()
    np.testing.assert_allclose(b.dgi, g("gi"), **tol)
    np.testing.assert_allclose(b.dgh, g("gh"), **tol)
    np.testing.assert_allclose(b.dgh_n, g("gh")[:, 2 * d:], **tol)
    assert np.array_equal(b.dgh[:, :2 * d], b.dgi[:, :2 * d])
    np.testing.assert_allclose(b.dpre, g("pre"), **tol)
    np.testing.assert_allclose(b.dagg, g("agg"), **tol)
    np.testing.assert_allclose(b.dh0, g("h0"), **tol)
    p = x["prev_idx"]
    if p is None:
        assert b.grad_prev is b.dh0
    elif x["n_old"]:
        np.testing.assert_allclose(b.grad_prev, g("hp"), **tol)
        assert np.array_equal(b.grad_prev[p[p >= 0]], b.dh0[p >= 0]) and b.grad_prev.shape == (x["n_old"], d)
    else:
        assert b.grad_prev.shape == (0, d)


@pytest.mark.parametrize("name", ["d20_tanh_mask", "d36_relu_mask", "d32_idd", "n17", "as5", "as16"])
def test_weight_gradients_equal_torch(name):
    """backward given agg (and Ws_next) == autograd of the same step in fp64 for every weight and bias gradient models._DenseStep returns,
    the projection's included: loss = <hidden, g> + <hidden Ws_next^T, g_as[:, :a]>; the pad columns of g_as carry values and change
    nothing."""
    case = dr.CASES[name]
    x = dr.inputs(case)
    d, a = case.d, case.attn_dim
    mask64 = None if x["mask"] is None else (x["mask"] > 0) / 0.75
    case = types.SimpleNamespace(**dict(vars(case), keep=0.75))
    x = dict(x, mask=mask64)
    T = _torch_step(case, x, mask64)
    loss = (T["hidden"] * torch.as_tensor(np.asarray(x["grad_hidden"], np.float64))).sum()
    extra = {}
    if a:
        g_as = np.random.default_rng(3).standard_normal((case.n, case.ap))
        Ws = torch.tensor(np.asarray(x["Ws_next"], np.float64), requires_grad=True)
        loss = loss + ((T["hidden"] @ Ws.T) * torch.as_tensor(g_as[:, :a])).sum()
        extra = dict(g_as=g_as, Ws_next=x["Ws_next"], hidden=T["hidden"].detach().numpy())
    loss.backward()
    f = dr.step_forward(case, x)
    b = dr.backward(x["grad_hidden"], f.ws.reshape(case.n, 5 * d), f.x, mask64, case.keep, case.act, x["W_h"], x["w_ih"], x["w_hh"], x["prev_idx"],
                    x["n_old"], agg=x["agg"], **extra)
    tol = dict(rtol=1e-10, atol=1e-11)
    for k in ("W_h", "w_ih", "w_hh", "b_ih", "b_hh"):
        np.testing.assert_allclose(getattr(b, "grad_" + k), T[k].grad.numpy(), err_msg=k, **tol)
        assert (b.S["grad_" + k] >= np.abs(getattr(b, "grad_" + k)) * (1 - 1e-12)).all()
    np.testing.assert_allclose(b.dagg, T["agg"].grad.numpy(), **tol)
    n_out, n_cs = 96 + 256 + 3, 96 + 256 + 3 + 4
    if a:
        np.testing.assert_allclose(b.grad_Ws, Ws.grad.numpy(), **tol)
        np.testing.assert_allclose(b.grad_hidden, np.asarray(x["grad_hidden"], np.float64) + g_as[:, :a] @ np.asarray(x["Ws_next"], np.float64), **tol)
        assert b.n["grad_Ws"] == n_out and b.n["dgi"] == a + 1 and b.n["dagg"] == 4 * d + a + 1 and b.n["grad_w_ih"] == a + 1 + n_out
    else:
        assert not hasattr(b, "grad_Ws") and b.n["grad_w_ih"] == b.n["grad_w_hh"] == n_out and b.n["grad_b_ih"] == b.n["grad_b_hh"] == n_cs
        assert b.n["grad_W_h"] == 3 * d + n_out and b.n["dgi"] == 0
    # without agg the function is what it was
    plain = dr.step_backward(case, x, f.x, f.ws.reshape(case.n, 5 * d))
    assert not hasattr(plain, "grad_W_h") and (a or np.array_equal(plain.dagg, b.dagg))


@functools.lru_cache(maxsize=None)
def _route_ratios(name, fault=None):
    """Per output: (worst ratio of the fp32 evaluation, share of its elements beyond the GPU's bound) on a route case, fed the fp64
    forward's x / ws / hidden rounded once."""
    case = dr.ROUTE_CASES[name]
    x = dr.inputs(case)
    f = dr.step_forward(case, x)
    xs, ws, hs = f.x.astype(np.float32), f.ws.astype(np.float32).reshape(case.n, 5 * case.d), f.hidden.astype(np.float32)
    b64, b32 = dr.route_backward(case, x, xs, ws, hs), dr.route_backward(case, x, xs, ws, hs, dtype=np.float32, fault=fault)
    r = {}
    for o in dr.WGRAD_OUTPUTS + ("dagg", "grad_prev", "grad_hidden"):
        if hasattr(b64, o):
            assert getattr(b32, o).dtype == np.float32 and getattr(b32, o).shape == getattr(b64, o).shape
            c = dr.C_BOUND_WGRAD if o in dr.WGRAD_OUTPUTS else dr.C_BOUND
            beyond = np.abs(getattr(b32, o).astype(np.float64) - getattr(b64, o)) > dr.bound(b64.S[o], b64.n[o], dr.N0_STEP, c)
            r[o] = (dr.worst_ratio(getattr(b32, o), getattr(b64, o), b64.S[o], b64.n[o], dr.N0_STEP), float(beyond.mean()) if beyond.size else 0.0)
    return r


@pytest.mark.parametrize("name", list(dr.ROUTE_CASES))
def test_fp32_weight_gradients_within_their_bound(name):
    """The weight and bias gradients evaluated in np.float32 - dgi / dgh / dpre in fp32, summed over the rows in rg_gram_tn's shape -
    against fp64 on every route case: the ratio stays below REF32_WORST_RATIO_WGRAD for every element (the GPU is allowed 4 x that);
    the row gradients of the same evaluation stay below REF32_WORST_RATIO, also where g itself is a sum (Ws_next).  Prints the ratios."""
    r = _route_ratios(name)
    print("%s: %s" % (name, " ".join("%s=%.3g" % (o, v[0]) for o, v in r.items())))
    assert ("grad_Ws" in r) == bool(dr.ROUTE_CASES[name].attn_dim) and set(dr.WGRAD_OUTPUTS[:5]) <= set(r)
    for o, (v, _) in r.items():
        assert v <= (dr.REF32_WORST_RATIO_WGRAD if o in dr.WGRAD_OUTPUTS else dr.REF32_WORST_RATIO), (name, o, v)


def test_recorded_weight_gradient_ratio_is_the_measured_one():
    """REF32_WORST_RATIO_WGRAD is the worst figure of the route table rounded up (bwd2_d64_as16's grad_Ws), within 1.25 x."""
    worst = max(v[0] for o, v in _route_ratios("bwd2_d64_as16").items() if o in dr.WGRAD_OUTPUTS)
    assert worst <= dr.REF32_WORST_RATIO_WGRAD <= 1.25 * worst and dr.C_BOUND_WGRAD == 4.0 * dr.REF32_WORST_RATIO_WGRAD, worst


@pytest.mark.parametrize("name", ["bwd2_d16", "bwd2_d20_as5", "bwd_d36"])
def test_bound_rejects_a_wrong_block_order(name):
    """grad_w_hh and grad_b_hh assembled as (n, r, z) blocks instead of (r, z, n) - torch.cat([g_n, g_rz]) in models.py:175 - fail the
    GPU's bound on most of their elements; every other gradient still passes."""
    r = _route_ratios(name, fault="cat_order")
    for o, (_, beyond) in r.items():
        if o in ("grad_w_hh", "grad_b_hh"):
            assert beyond > (0.5 if o == "grad_b_hh" or dr.ROUTE_CASES[name].prev != "none" else -1), (o, beyond)
        else:
            assert beyond == 0.0, (o, beyond)


def test_route_table_covers_what_it_names():
    C = list(dr.ROUTE_CASES.values())
    assert all(c.kind == "route" and c.why and "models.py:" in c.why for c in C) and not set(dr.ROUTE_CASES) & set(dr.CASES)
    bwd2 = [c for c in C if c.name.startswith("bwd2_")]
    assert {c.d for c in bwd2 if not c.attn_dim} == set(range(16, 65, 4)) and all(c.n == 32768 and c.prev == "third" for c in bwd2)
    assert {(c.d, c.attn_dim) for c in bwd2 if c.attn_dim} == {(d, a) for d in (20, 48, 64) for a in (5, 16)}
    assert {c.act for c in bwd2} == {0, 1, 2} and {c.masked for c in bwd2} == {True, False}
    assert {(c.d, c.n, c.prev) for c in C if c.name.startswith("bwd_")} == {(d, 32768, "none") for d in (16, 36, 64)}
    assert {(c.name, c.d, c.n) for c in C if not c.name.startswith("bwd")} == {("sums_n8192", 32, 8192), ("sums_n32767", 32, 32767),
                                                                               ("aten_n8191", 32, 8191), ("aten_d128", 128, 32768)}
    why = " ".join(c.why for c in C)      # the four places of _DenseStep.backward that reach engine.gram_tn
    for line in ("models.py:164", "models.py:172-174", "models.py:180-182", "models.py:201-202", "models.py:68", "models.py:175", "models.py:185",
                 "models.py:187"):
        assert line in why, line
    x = dr.inputs(dr.ROUTE_CASES["bwd2_d20_as5"])
    assert x["g_as"].shape == (32768, 8) and np.abs(x["g_as"][:, 5:]).min() > 0 and x["n_old"] == (32768 + 2) // 3
    x = dr.inputs(dr.ROUTE_CASES["bwd_d16"])
    assert x["n_old"] == 0 and (x["prev_idx"] == -1).all()


def test_rows_products_against_numpy():
    for name in ("am32_k5", "am64_k32"):
        c = dr.CASES[name]
        x = dr.inputs(c)
        base = x["base"][:, :c.cols]
        want = base.astype(np.float64) + x["g"][:, :c.k].astype(np.float64) @ x["W"].astype(np.float64)
        np.testing.assert_allclose(dr.rows_addmm(base, x["g"], x["W"]).out, want, rtol=1e-13, atol=1e-13)
    c = dr.CASES["t3_d30_ld32"]
    x = dr.inputs(c)
    t = dr.attn_tables(x["rela"][1], x["Wr"][1], x["Wqr"][1], x["bqr"][1], x["q_rel"], c.ap, c.ld)
    lin = torch.nn.functional.linear
    T = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    np.testing.assert_allclose(t.a_r[:, :3], lin(T(x["rela"][1]), T(x["Wr"][1])).numpy(), rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(t.a_q[:, :3], lin(T(x["rela"][1])[x["q_rel"]], T(x["Wqr"][1]), T(x["bqr"][1])).numpy(), rtol=1e-13, atol=1e-13)
    assert not t.a_r[:, 3:].any() and not t.a_q[:, 3:].any() and not t.rela_pad[:, 30:].any() and not t.S["a_q"][:, 3:].any()
    assert np.array_equal(t.rela_pad[:, :30], x["rela"][1].astype(np.float64)) and t.rela_pad.shape == (c.n_rows, 32)


def test_table_covers_what_it_names():
    """The table really contains the conditions its comments name."""
    C = list(dr.CASES.values())
    st = [c for c in C if c.kind == "step"]
    assert {c.d for c in st if not c.fwd_only} == {16, 20, 32, 36, 48, 60, 64} and {c.d for c in st if c.fwd_only} == {128}
    for nb2 in (True, False):      # both backward templates see every activation, a mask and no mask
        sub = [c for c in st if not c.fwd_only and (c.d <= 32) == nb2]
        assert {c.act for c in sub} == {0, 1, 2} and {c.masked for c in sub} == {True, False}
        assert {c.prev for c in sub} >= {"third", "all"}
    assert {c.prev for c in st} == {"null", "none", "third", "all"} and {c.act for c in st if c.fwd_only} == {0, 1, 2}
    ns = {c.n for c in st}
    assert {1, 15, 16, 17, 8191, 8193, 32767, 32769} <= ns and max(ns) > 2 * 256 * 8 * 16
    assert {c.d for c in st if c.n > 2 * 256 * 8 * 16} == {20, 64, 128}
    assert {c.attn_dim for c in st} == {0, 1, 5, 8, 16} and any(c.attn_dim and c.d == 128 for c in st)
    for c in st:
        x = dr.inputs(c)
        p = x["prev_idx"]
        if c.prev == "null":
            assert p is None and x["hidden_prev"] is None
        elif c.prev == "none":
            assert (p == -1).all() and x["n_old"] == 0
        else:
            old = p[p >= 0]
            assert x["n_old"] == (c.n if c.prev == "all" else (c.n + 2) // 3) == len(old) and np.array_equal(np.sort(old), np.arange(len(old)))
            assert x["hidden_prev"].shape == (x["n_old"], c.d)
        if c.masked:
            m = x["mask"]
            assert set(np.unique(m)) <= {np.float32(0), np.float32(1) / np.float32(0.7)} and (c.n * c.d < 100 or 0.5 < (m > 0).mean() < 0.9)
        else:
            assert x["mask"] is None
    am = [c for c in C if c.kind == "addmm"]
    assert {c.cols for c in am} == {16, 32, 48, 64, 128} and {c.k for c in am} == {1, 5, 16, 32}
    assert any(c.g_width > c.k for c in am) and any(c.base_width > c.cols and c.g_width > c.k for c in am) and any(c.alias for c in am)
    assert any(256 % (c.cols // 4) for c in am) and max(c.n_rows for c in am) > 2048 * 21
    tb = [c for c in C if c.kind == "tables"]
    assert {c.n_layer for c in tb} == {1, 3, 5} and {(c.d, c.ld) for c in tb} >= {(64, 64), (30, 32), (48, 64)}
    assert {c.attn_dim for c in tb} == {3, 5, 16} and all(c.ap > c.attn_dim for c in tb) and any(c.n_rows == 475 for c in tb)
    for c in tb:
        q = dr.inputs(c)["q_rel"]
        assert len(np.unique(q)) < len(q) and q.max() == c.n_rows - 1
    assert all(c.why for c in C)


@functools.lru_cache(maxsize=2)
def _infer_ref(name):
    """(inputs, fp64 reference) of an inference case, shared by the tests that follow one another on it."""
    case = dr.INFER_CASES[name]
    x = dr.infer_inputs(case)
    return x, dr.infer_forward(case, x)


def _outputs(f64):
    return [o for o in dr.INFER_OUTPUTS if getattr(f64, o) is not None]


def _ratios(case):
    r = {}
    if case.kind == "infer":
        x, f64 = _infer_ref(case.name)
        f32 = dr.infer_forward(case, x, dtype=np.float32)
        assert f32.hidden.dtype == np.float32 and (f32.score is None or f32.score.dtype == np.float32)
        for o in _outputs(f64):
            r[o] = dr.worst_ratio(getattr(f32, o), getattr(f64, o), f64.S[o], f64.n[o], dr.N0_STEP)
        return r
    x = dr.inputs(case)
    if case.kind == "step":
        f64, f32 = dr.step_forward(case, x), dr.step_forward(case, x, dtype=np.float32)
        assert f32.hidden.dtype == f32.ws.dtype == np.float32
        for o in dr.FWD_OUTPUTS:
            if getattr(f64, o) is not None:
                r[o] = dr.worst_ratio(getattr(f32, o), getattr(f64, o), f64.S[o], f64.n[o], dr.N0_STEP)
        if not case.fwd_only:
            xs, ws = dr.saved(case, x)
            b64, b32 = dr.step_backward(case, x, xs, ws), dr.step_backward(case, x, xs, ws, dtype=np.float32)
            assert b32.dagg.dtype == np.float32
            for o in dr.BWD_OUTPUTS:
                r[o] = dr.worst_ratio(getattr(b32, o), getattr(b64, o), b64.S[o], b64.n[o], dr.N0_STEP)
    elif case.kind == "addmm":
        a = (x["base"][:, :case.cols], x["g"], x["W"])
        a64, a32 = dr.rows_addmm(*a), dr.rows_addmm(*a, dtype=np.float32)
        r["out"] = dr.worst_ratio(a32.out, a64.out, a64.S["out"], a64.n["out"], dr.N0_ROWS)
    else:
        for l in range(case.n_layer):
            a = (x["rela"][l], x["Wr"][l], x["Wqr"][l], x["bqr"][l], x["q_rel"], case.ap, case.ld)
            t64, t32 = dr.attn_tables(*a), dr.attn_tables(*a, dtype=np.float32)
            for o in ("a_r", "a_q"):
                r[o] = max(r.get(o, 0.0), dr.worst_ratio(getattr(t32, o), getattr(t64, o), t64.S[o], t64.n[o], dr.N0_ROWS))
    return r


_BOTH_TABLES = [pytest.param(c, id=c.name) for c in dr.CASES.values()] + [pytest.param(c, id="infer-" + c.name) for c in dr.INFER_CASES.values()]


@pytest.mark.parametrize("case", _BOTH_TABLES)
def test_fp32_reference_within_its_bound(case):
    """The reference evaluated in np.float32 (same code, same order) against its fp64 self on every case of both tables (the inference
    table: hidden, a_s and score): the ratio |ref32 - ref64| / ((n + n0) u S) stays below the recorded constant for every element of
    every output, i.e. the GPU's bound (4 x that) is one a correct fp32 implementation meets with a factor 4 to spare.  Prints the
    ratios."""
    name = case.name
    r = _ratios(case)
    print("%s: %s" % (name, " ".join("%s=%.3g" % kv for kv in r.items())))
    limit = dr.REF32_WORST_RATIO if case.kind in ("step", "infer") else dr.REF32_WORST_RATIO_ROWS
    for o, v in r.items():
        assert v <= limit, (name, o, v)


def test_recorded_ratios_are_the_measured_ones():
    """The recorded constants are the table's worst figures rounded up, not a looser guess: each lies within 1.25 x of what its worst
    case measures (n70001_d64's dgi, am16_k1's out)."""
    step = max(_ratios(dr.CASES["n70001_d64"]).values())
    rows = max(_ratios(dr.CASES["am16_k1"]).values())
    assert step <= dr.REF32_WORST_RATIO <= 1.25 * step and rows <= dr.REF32_WORST_RATIO_ROWS <= 1.25 * rows, (step, rows)
    # the inference table's worst fp32 figure (w_d1_ld4's hidden, 0.049; its worst score 0.040) lies below the step's: the table shares
    # REF32_WORST_RATIO and needs no constant of its own
    infer = _ratios(dr.INFER_CASES["w_d1_ld4"])
    assert max(infer.values()) <= dr.REF32_WORST_RATIO and 0 < infer["score"] <= dr.REF32_WORST_RATIO, infer
    # the two-term emulation's constant: spike_d20_ld32's hidden
    f16x2 = max(_f16x2_ratios(dr.INFER_CASES["spike_d20_ld32"]).values())
    assert f16x2 <= dr.REF_F16X2_WORST_RATIO <= 1.25 * f16x2 and dr.C2_F16X2 == 2.0 * dr.REF_F16X2_WORST_RATIO, f16x2


def _f16x2_ratios(case, fault=None):
    """|forward_f16x2 - ref64| / (p 2^-22 S), the worst element per output."""
    x, f64 = _infer_ref(case.name)
    e = dr.infer_forward_f16x2(case, x, fault=fault)
    r = {}
    for o in _outputs(f64):
        err = np.abs(getattr(e, o) - getattr(f64, o))
        den = dr.P_CHAIN[o] * dr.U22 * f64.S[o]
        with np.errstate(divide="ignore", invalid="ignore"):
            r[o] = float(np.where(den > 0, err / den, np.where(err > dr.TINY, np.inf, 0.0)).max())
    return r


@pytest.mark.parametrize("name", list(dr.INFER_CASES))
def test_f16x2_emulation_within_its_recorded_ratio(name):
    """The two-term operand form emulated in numpy (dr.forward_f16x2) against the fp64 reference on every inference case: the ratio
    |emul - ref64| / (p 2^-22 S) stays below REF_F16X2_WORST_RATIO for every element of every output; precision 1's added allowance is
    2 x that.  Prints the ratios."""
    r = _f16x2_ratios(dr.INFER_CASES[name])
    print("%s: %s" % (name, " ".join("%s=%.3g" % kv for kv in r.items())))
    for o, v in r.items():
        assert v <= dr.REF_F16X2_WORST_RATIO, (name, o, v)


@pytest.mark.parametrize("fault,case_name,outputs", [("no_b_hn", "d48_tanh", ("ws", "hidden")), ("no_b_hn", "d20_tanh_mask", ("ws", "hidden")),
                                                     ("dgh_n_no_r", "d64_relu_mask", ("dgh", "dgh_n", "dh0", "grad_prev")),
                                                     ("dgh_n_no_r", "d16_relu", ("dgh", "dgh_n", "dh0", "grad_prev")),
                                                     ("col_shift", "d36_relu_mask", ("dgi", "dgh", "dpre", "dagg", "dh0")),
                                                     ("no_lo_hi", "w_d20", ("hidden", "a_s", "score")),
                                                     ("no_lo_hi", "w_d3_ld4", ("hidden", "a_s", "score")),
                                                     ("one_term", "w_d20", ("hidden", "a_s", "score")),
                                                     ("stale_all_new", "prev_runs_d64", ("hidden", "a_s")),
                                                     ("stale_all_new", "w_d128", ("hidden", "a_s", "score")),
                                                     ("readout_h0", "readout", ("score",)),
                                                     ("readout_h0", "w_d1_ld4", ("score",))])
def test_bound_rejects_a_wrong_kernel(fault, case_name, outputs):
    """The tests can fail: the reference's own fp32 copy of the operation with one thing wrong - one gate bias (b_hn) dropped; dgh's n
    block missing its * r; at d = 36 the partly filled column block reading z one column to the right - is rejected by the GPU's bound
    on each output the fault reaches (on more than 1 % of its elements, not on a stray one); the outputs upstream of the fault still pass.
    The inference table: the two-term emulation with its W_lo X_hi term dropped, and with a single f16 term, fails PRECISION 1's bound
    (the added 2^-22 term has not swallowed what the bound is for; at d = 128 the common term alone is wider than an 11-bit operand's
    error, which is why the bit-for-bit product test of tests/test_dense_infer_gpu.py exists); an fp32 evaluation whose all-new tiles
    keep the last mixed tile's h0, and one whose readout reads h0 instead of the new state, fail the common bound."""
    if fault in ("no_lo_hi", "one_term", "stale_all_new", "readout_h0"):
        case = dr.INFER_CASES[case_name]
        x, ref = _infer_ref(case_name)
        two_term = fault in ("no_lo_hi", "one_term")
        bad = dr.infer_forward_f16x2(case, x, fault=fault) if two_term else dr.infer_forward(case, x, dtype=np.float32, fault=fault)
        if fault == "stale_all_new":
            assert min(dr.tile_census(x["prev_idx"], case.n)) > 0
        for o in _outputs(ref):
            within = np.abs(np.asarray(getattr(bad, o), np.float64) - getattr(ref, o)) <= dr.infer_bound(1 if two_term else 0, ref.S[o],
                                                                                                         ref.n[o], o)
            if o in outputs:
                assert (~within).mean() > 0.01, (o, (~within).mean())
            elif fault == "readout_h0":
                assert within.all(), o      # the state and a_s are upstream of the readout
        return
    case = dr.CASES[case_name]
    x = dr.inputs(case)
    if fault == "no_b_hn":
        ref, bad = dr.step_forward(case, x), dr.step_forward(case, x, dtype=np.float32, fault=fault)
        names, clean = dr.FWD_OUTPUTS, ("x",)
    else:
        xs, ws = dr.saved(case, x)
        ref, bad = dr.step_backward(case, x, xs, ws), dr.step_backward(case, x, xs, ws, dtype=np.float32, fault=fault)
        names, clean = dr.BWD_OUTPUTS, () if fault == "col_shift" else ("dgi", "dpre", "dagg")
    for o in names:
        if getattr(ref, o) is None:
            continue
        within = np.abs(getattr(bad, o).astype(np.float64) - getattr(ref, o)) <= dr.bound(ref.S[o], ref.n[o], dr.N0_STEP, dr.C_BOUND)
        if o in outputs:
            assert (~within).mean() > 0.01, (o, (~within).mean())      # col_shift reaches 4 of dgi's 108 columns: 3.7 %
        elif o in clean:
            assert within.all(), o


# ---- the inference table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w_d3_ld4", "w_d20", "w_d33_ld36", "prev_runs_d64", "readout", "prev_null", "n1_d128"])
def test_inference_reference_equals_torch(name):
    """The extended forward == torch.gru_cell around the same W_h / carry in fp64, a_s == hidden Ws^T, score == hidden . W_final with
    S_score = S_hidden |W_final| and n_score = n_hidden + d, and the scatter helper puts score m at nodes[m, 0] * n_ent + nodes[m, 1]."""
    case = dr.INFER_CASES[name]
    x, f = _infer_ref(name)
    d, n = case.d, case.n
    step = types.SimpleNamespace(d=d, n=n, act=case.act)
    T = _torch_step(step, dict(x, mask=None), None)
    tol = dict(rtol=1e-11, atol=1e-12)
    hidden = T["cell"].detach().numpy()
    np.testing.assert_allclose(f.hidden, hidden, **tol)
    if case.attn_dim:
        np.testing.assert_allclose(f.a_s[:, :case.attn_dim], hidden @ np.asarray(x["Ws_next"], np.float64).T, **tol)
        assert f.a_s.shape == (n, case.ap) and not f.a_s[:, case.attn_dim:].any() and not f.S["a_s"][:, case.attn_dim:].any()
    else:
        assert f.a_s is None and "a_s" not in f.S
    if not case.readout:
        assert f.score is None and "score" not in f.S
        return
    w = np.asarray(x["W_final"], np.float64)
    np.testing.assert_allclose(f.score, torch.as_tensor(hidden) @ torch.as_tensor(w), **tol)
    np.testing.assert_allclose(f.S["score"], f.S["hidden"] @ np.abs(w), rtol=1e-14)
    assert f.n["score"] == f.n["hidden"] + d == f.n.get("a_s", f.n["score"]) and f.score.shape == (n,)
    nodes, n_ent, size = x["nodes"], x["n_ent"], x["n_scores"]
    all_ = dr.scatter_scores(f.score, nodes, n_ent, size)
    at = nodes[:, 0].astype(np.int64) * n_ent + nodes[:, 1]
    assert np.array_equal(all_[at], f.score) and np.isnan(all_).sum() == size - n
    # sorted distinct pairs with gaps: not an arange
    assert (np.diff(at) > 0).all() and at.max() < size and (n < 16 or (np.diff(at) > 1).any()) and (nodes[:, 1] < n_ent).all()


def test_runs_mode_has_every_kind_of_tile():
    """prev_idx of every `runs` case really holds 16-row tiles without an old row, tiles of old rows only and mixed tiles (the all-new
    branch of any_old next to mixed tiles inside one call); a third at random has (almost) only mixed ones."""
    runs = [c for c in dr.INFER_CASES.values() if c.prev == "runs"]
    assert {c.d for c in runs} >= {1, 20, 30, 33, 63, 64, 128}
    for c in runs:
        x = dr.infer_inputs(c)
        p = x["prev_idx"]
        new, old, mixed = dr.tile_census(p, c.n)
        assert new >= 5 and old >= 5 and mixed >= 5 and new + old + mixed == (c.n + 15) // 16, (c.name, new, old, mixed)
        # somewhere an all-new tile sits right behind a tile with old rows (a stale h0 would have something to be stale with)
        has_old = np.array([(p[t:t + 16] >= 0).any() for t in range(0, c.n, 16)])
        assert (has_old[:-1] & ~has_old[1:]).any() and (~has_old[:-1] & has_old[1:]).any()
        sel = np.sort(p[p >= 0])
        assert x["n_old"] == len(sel) and np.array_equal(sel, np.arange(len(sel))) and x["hidden_prev"].shape == (max(len(sel), 1), c.d)
        runs_len = np.diff(np.flatnonzero(np.diff(np.r_[-1, (p >= 0).astype(int), -1]) != 0))
        assert 1 <= runs_len.min() and runs_len.max() <= 40
    c = dr.INFER_CASES["prev_third"]
    assert dr.tile_census(dr.infer_inputs(c)["prev_idx"], c.n)[0] == 0
    assert dr.tile_census(None, 33) == (3, 0, 0) and dr.tile_census(np.zeros(33, np.int32), 33) == (0, 3, 0)


def test_inference_table_covers_what_it_names():
    C = list(dr.INFER_CASES.values())
    assert all(c.why and c.kind == "infer" for c in C) and not set(dr.INFER_CASES) - {c.name for c in C}
    wide = {(c.d, c.ld) for c in C if c.n == 1000 and c.rows == "plain" and c.attn_dim and c.readout}
    assert wide >= {(1, 4), (3, 4), (20, 20), (20, 32), (30, 32), (32, 32), (33, 36), (48, 64), (63, 64), (64, 64), (128, 128)}
    assert all(c.ld >= c.d and c.ld % 4 == 0 and c.ld <= 128 and c.ap == (c.attn_dim + 3) // 4 * 4 for c in C)
    for d in (64, 128):
        assert {c.n for c in C if c.d == d} >= {1, 15, 16, 17}
    # a second pass of the persistent grid, per kernel: rows per pass from its NW
    assert dr.ROWS_PER_PASS == {8: 32768, 4: 16384}
    big = {(c.d, c.n, c.precisions) for c in C if c.n > 16384}
    assert big == {(64, 32769, (0, 1, 2)), (20, 32769, (0, 1, 2)), (128, 32769, (0, 1)), (128, 16385, (2,))}
    assert all(c.precisions == (0, 1, 2) for c in C if c.n <= 16384)
    assert {c.prev for c in C} == {"null", "none", "all", "third", "runs"}
    assert {c.attn_dim for c in C} == {0, 1, 5, 8, 16} and {c.ap for c in C} == {0, 4, 8, 16}
    for d128 in (True, False):
        sub = [c for c in C if (c.d == 128) == d128]
        assert {c.act for c in sub} == {0, 1, 2} and {c.prev for c in sub} >= {"runs", "third", "all"}
        assert any(c.readout and not c.attn_dim for c in sub) and any(not c.readout and not c.attn_dim for c in sub)
        assert any(c.no_hidden for c in sub) and any(c.attn_dim == 16 for c in sub) and any(c.ws_scale == 300.0 for c in sub)
        assert {c.rows for c in sub} == {"plain", "spike", "x_over_h", "h_over_x"}
    assert all(c.readout and not c.attn_dim for c in C if c.no_hidden)
    assert all(c.act == 0 and c.prev in ("runs", "third") for c in C if c.rows in ("x_over_h", "h_over_x"))
    # the spike: one element 8 x the row's largest other one, its column cycling over all d; rows spread over five decades
    c = dr.INFER_CASES["spike_d64"]
    a = np.abs(dr.infer_inputs(c)["agg"].astype(np.float64))
    col = a.argmax(1)
    assert np.array_equal(col, np.arange(c.n) % c.d)
    rest = np.where(np.arange(c.d)[None] == col[:, None], 0.0, a).max(1)
    ratio = a.max(1) / rest      # 8 x the noise row's largest; more where that largest sat in the spike's own column
    assert (ratio > 8.0 * (1 - 1e-6)).all() and (np.abs(ratio - 8.0) < 1e-5).mean() > 0.95
    assert a.max(1).max() / a.max(1).min() > 1e4 and a.max() * 2.0 ** 14 / 2.0 ** np.floor(np.log2(a.max())) < 65504
    x = dr.infer_inputs(dr.INFER_CASES["x_over_h_d64"])
    assert np.abs(x["agg"]).mean() > 50 * np.abs(x["hidden_prev"]).mean()
    x = dr.infer_inputs(dr.INFER_CASES["h_over_x_d64"])
    assert np.abs(x["agg"]).mean() * 50 < np.abs(x["hidden_prev"]).mean()
    x = dr.infer_inputs(dr.INFER_CASES["ws300_d64"])
    assert np.abs(x["Ws_next"]).max() > 100 * np.abs(x["w_ih"]).max()


def test_two_term_split_by_hand():
    """hi + lo of the emulated operand form carries 22 bits: v = 1 + 2^-12 + 2^-21 at scale 2^14 splits into hi = 2^14 (f16 has 11
    bits), lo = 4 + 2^-7 exactly; 2^-23 more is beyond lo's 11 bits and is rounded away.  Scales: 3 -> 2^13 (row), 2^12 (weights)."""
    hi, lo = dr._split2(np.array([1 + 2.0 ** -12 + 2.0 ** -21, 1 + 2.0 ** -12 + 2.0 ** -21 + 2.0 ** -25]), 2.0 ** 14)
    assert hi.tolist() == [2.0 ** 14, 2.0 ** 14] and lo.tolist() == [4 + 2.0 ** -7, 4 + 2.0 ** -7]
    assert dr._pow2_scale(3.0, 15) == 2.0 ** 13 and dr._pow2_scale(3.0, 14) == 2.0 ** 12 and dr._pow2_scale(0.0, 15) == 1.0
    assert dr._pow2_scale(2.0 ** 14, 15) == 1.0 and dr._pow2_scale(np.nextafter(2.0 ** 15, 0), 15) == 1.0
    X, W = np.array([[3.0, 0.5]]), np.array([[0.25, 2.0]])
    assert dr._prod2(X, 2.0 ** 13, W, 2.0 ** 12)[0, 0] == 1.75      # exactly representable operands: the product is exact
