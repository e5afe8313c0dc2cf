"""The dense-step reference (tests/dense_ref.py) checked on the CPU: by hand, against torch.gru_cell and torch autograd in fp64, its own
fp32 evaluation against the bound the GPU tests use (so the bound is known to be satisfiable by a correct fp32 implementation before a
GPU is involved), and the bound against three deliberately wrong copies of the operation (so it is known to reject a subtly wrong
kernel)."""
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
    return dict(agg=agg, hp=hp, h0=h0, pre=pre, x=xx, gi=gi, gh=gh, r=r, z=z, ng=ng, hidden=hidden, cell=cell)


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


def _ratios(case):
    x = dr.inputs(case)
    r = {}
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


@pytest.mark.parametrize("name", list(dr.CASES))
def test_fp32_reference_within_its_bound(name):
    """The reference evaluated in np.float32 (same code, same order) against its fp64 self on every case of the table: the ratio
    |ref32 - ref64| / ((n + n0) u S) stays below the recorded constant for every element of every output, i.e. the GPU's bound
    (4 x that) is one a correct fp32 implementation meets with a factor 4 to spare.  Prints the ratios."""
    case = dr.CASES[name]
    r = _ratios(case)
    print("%s: %s" % (name, " ".join("%s=%.3g" % kv for kv in r.items())))
    limit = dr.REF32_WORST_RATIO if case.kind == "step" else dr.REF32_WORST_RATIO_ROWS
    for o, v in r.items():
        assert v <= limit, (name, o, v)


def test_recorded_ratios_are_the_measured_ones():
    """The recorded constants are the table's worst figures rounded up, not a looser guess: each lies within 1.25 x of what its worst
    case measures (n70001_d64's dgi, am16_k1's out)."""
    step = max(_ratios(dr.CASES["n70001_d64"]).values())
    rows = max(_ratios(dr.CASES["am16_k1"]).values())
    assert step <= dr.REF32_WORST_RATIO <= 1.25 * step and rows <= dr.REF32_WORST_RATIO_ROWS <= 1.25 * rows, (step, rows)


@pytest.mark.parametrize("fault,case_name,outputs", [("no_b_hn", "d48_tanh", ("ws", "hidden")), ("no_b_hn", "d20_tanh_mask", ("ws", "hidden")),
                                                     ("dgh_n_no_r", "d64_relu_mask", ("dgh", "dgh_n", "dh0", "grad_prev")),
                                                     ("dgh_n_no_r", "d16_relu", ("dgh", "dgh_n", "dh0", "grad_prev")),
                                                     ("col_shift", "d36_relu_mask", ("dgi", "dgh", "dpre", "dagg", "dh0"))])
def test_bound_rejects_a_wrong_kernel(fault, case_name, outputs):
    """The tests can fail: the reference's own fp32 copy of the operation with one thing wrong - one gate bias (b_hn) dropped; dgh's n
    block missing its * r; at d = 36 the partly filled column block reading z one column to the right - is rejected by the GPU's bound
    on each output the fault reaches (on more than 1 % of its elements, not on a stray one); the outputs upstream of the fault still pass."""
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
