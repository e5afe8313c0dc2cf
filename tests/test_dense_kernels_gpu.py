"""The dense training kernels called on their own - rg_dense_train_fwd / _fwd_as, rg_dense_train_bwd / _bwd2, rg_rows_addmm,
rg_attn_tables - against the fp64 reference of tests/dense_ref.py, over the case table defined there (one case per dispatch condition;
each case's ``why`` cites the condition it flips).  Every output buffer the header calls WRITTEN is pre-filled with NaN and must be
written completely; then every element of every output (nothing exempt) must satisfy

    |gpu - ref64| <= C * (n + n0) * u * S + 1e-30                (dense_ref's docstring defines S, n, n0)

with C = dense_ref.C_BOUND = 4 x 0.3 = 1.2 for the step and C_BOUND_ROWS = 4 x 0.6 = 2.4 for the two row-wise products: 4 x what the
plain-numpy fp32 evaluation of the reference costs on these cases (tests/test_dense_ref.py::test_fp32_reference_within_its_bound keeps
those figures honest on the CPU).  The backward kernels are fed the fp64 forward's x / ws rounded once, the same arrays the reference
reads, so a backward failure cannot be a forward error in disguise.  The kernels' own worst ratios are printed per case (run with -s)
and summarised in KERNEL_RATIOS below, for information only.
"""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import dense_ref as dr

pytestmark = pytest.mark.gpu

# the kernels' worst |gpu - ref64| / ((n + n0) u S) per output over the whole table, as measured on an MI355X (information only; the
# assertions use C_BOUND / C_BOUND_ROWS)
KERNEL_RATIOS = {"hidden": 0.031, "x": 0.163, "ws": 0.164, "a_s": 0.0046, "dgi": 0.274, "dgh": 0.274, "dgh_n": 0.237, "dpre": 0.019,
                 "dagg": 0.0067, "dh0": 0.018, "grad_prev": 0.018, "rows_addmm out": 0.46, "a_r": 0.048, "a_q": 0.052}
# wall time of this file on an MI355X: 9.6 s (37 tests)

NAN = float("nan")


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _check(what, gpu, ref, S, n, n0, c):
    """Every element of ``gpu`` written and within the bound of ``ref``.  Returns the worst ratio."""
    gpu = gpu.detach().cpu().numpy().astype(np.float64).reshape(np.shape(ref))
    assert not np.isnan(gpu).any(), "%s: %d elements were never written" % (what, int(np.isnan(gpu).sum()))
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    ok = np.abs(gpu - ref) <= dr.bound(S, n, n0, c)
    ratio = dr.worst_ratio(gpu, ref, S, n, n0)
    nn = np.broadcast_to(np.asarray(n, np.float64), ref.shape)
    assert ok.all(), ("%s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g); first at %s: gpu %.9g ref %.9g S %.3g n %d"
                      % (what, int((~ok).sum()), ok.size, ratio, c, np.argwhere(~ok)[0], gpu[~ok][0], ref[~ok][0], S[~ok][0], int(nn[~ok][0])))
    return ratio


def _gate(X):
    return types.SimpleNamespace(weight_ih_l0=X["w_ih"], weight_hh_l0=X["w_hh"], bias_ih_l0=X["b_ih"], bias_hh_l0=X["b_hh"])


def _upload(case, x):
    X = {k: _dev(v) for k, v in x.items() if k not in ("prev_idx", "n_old")}
    X["prev_idx"] = _dev(x["prev_idx"], torch.int32)
    return X


def _fwd(case, X, mask, with_as):
    """rg_dense_train_fwd / rg_dense_train_fwd_as into NaN-filled outputs: (hidden, x, ws [n, 5 d], a_s or None)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, d = case.n, case.d
    hidden, xo, ws = _nan(n, d), _nan(n, d), _nan(n, 5 * d)
    common = (n, d, p(X["agg"]), p(X["hidden_prev"]), p(X["prev_idx"]), p(X["W_h"]), case.act, p(X["w_ih"]), p(X["w_hh"]), p(X["b_ih"]),
              p(X["b_hh"]), p(mask))
    if not with_as:
        _lib.check(L.rg_dense_train_fwd(*common, p(hidden), p(xo), p(ws), _lib.stream_ptr()))
        return hidden, xo, ws, None
    a_s = _nan(n, case.ap)
    _lib.check(L.rg_dense_train_fwd_as(*common, p(X["Ws_next"]), case.attn_dim, case.ap, p(hidden), p(xo), p(ws), p(a_s), _lib.stream_ptr()))
    return hidden, xo, ws, a_s


def _bwd(case, X, xs, ws, n_old, two):
    """rg_dense_train_bwd (dgi, dgh, dpre, dagg, dh0) or rg_dense_train_bwd2 (dgi, dgh_n, dpre, dagg, grad_prev) into NaN-filled
    outputs.  grad_prev has n_old rows (one untouched row when no node is old: a NULL pointer is an argument error)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, d = case.n, case.d
    head = (n, d, p(X["grad_hidden"]), p(ws), p(xs), p(X["mask"]), case.keep, case.act, p(X["W_h"]), p(X["w_ih"]), p(X["w_hh"]))
    dgi, dpre, dagg = _nan(n, 3 * d), _nan(n, d), _nan(n, d)
    if not two:
        dgh, dh0 = _nan(n, 3 * d), _nan(n, d)
        _lib.check(L.rg_dense_train_bwd(*head, p(dgi), p(dgh), p(dpre), p(dagg), p(dh0), _lib.stream_ptr()))
        return dict(dgi=dgi, dgh=dgh, dpre=dpre, dagg=dagg, dh0=dh0)
    dgh_n = _nan(n, d)
    g_prev = _nan(n if X["prev_idx"] is None else max(n_old, 1), d)
    _lib.check(L.rg_dense_train_bwd2(*head, p(X["prev_idx"]), p(dgi), p(dgh_n), p(dpre), p(dagg), p(g_prev), _lib.stream_ptr()))
    return dict(dgi=dgi, dgh_n=dgh_n, dpre=dpre, dagg=dagg, grad_prev=g_prev)


def _step_case(case):
    from red_gnn_amd import _lib, engine as eng
    L, p = _lib.lib(), _lib.ptr
    x = dr.inputs(case)
    X = _upload(case, x)
    n, d, name = case.n, case.d, case.name
    act = {v: k for k, v in dr.ACT.items()}[case.act]
    ratios = {}

    # ---- forward: all of hidden, x, the five workspace blocks (and a_s) written and within the bound
    f64 = dr.step_forward(case, x)
    hidden, xo, ws, _ = _fwd(case, X, X["mask"], False)
    outs = dict(hidden=hidden, x=xo, ws=ws)
    if case.attn_dim:
        h2, x2, w2, a_s = _fwd(case, X, X["mask"], True)
        assert torch.equal(h2, hidden) and torch.equal(x2, xo) and torch.equal(w2, ws), name + ": _fwd_as differs from _fwd"
        outs["a_s"] = a_s
        assert not a_s[:, case.attn_dim:].any(), name + ": pad columns of a_s"
    for o, t in outs.items():
        ratios[o] = _check("%s %s" % (name, o), t, getattr(f64, o), f64.S[o], f64.n[o], dr.N0_STEP, dr.C_BOUND)
    # the carried state is a copy
    assert np.array_equal(ws.view(n, 5, d)[:, 3].cpu().numpy(), f64.ws[:, 3].astype(np.float32)), name + ": h0 block"
    # second run, through the engine wrapper: bitwise the same
    again = eng.dense_train_fwd(X["agg"], X["hidden_prev"], X["prev_idx"], X["W_h"], act, _gate(X), X["mask"], X["Ws_next"])
    for t, u in zip(again, (hidden, xo, ws, outs.get("a_s"))):
        assert (t is None and u is None) or torch.equal(t, u), name + ": second forward run differs"
    # mask = NULL: the training kernel's new state is the inference kernel's (precision 0) bit for bit - dense.hip launch<NB, true> and
    # launch<NB, false>, dense128_kernel<true> and <false>, are one body
    h_train = hidden if X["mask"] is None else _fwd(case, X, None, False)[0]
    h_inf = _nan(n, d)
    _lib.check(L.rg_dense_fwd(n, d, d, p(X["agg"]), p(X["hidden_prev"]), p(X["prev_idx"]), p(X["W_h"]), case.act, p(X["w_ih"]), p(X["w_hh"]),
                              p(X["b_ih"]), p(X["b_hh"]), None, 0, 0, None, None, None, 0, None, p(h_inf), 0, None, 0, _lib.stream_ptr()))
    assert torch.equal(h_train, h_inf), name + ": rg_dense_train_fwd(mask = NULL) differs bitwise from rg_dense_fwd(precision 0)"
    if case.fwd_only:
        return ratios

    # ---- backward, both entries, on the saved x / ws of the fp64 forward rounded once
    xs_np, ws_np = dr.saved(case, x)
    xs, wsd = _dev(xs_np), _dev(ws_np)
    b64 = dr.step_backward(case, x, xs_np, ws_np)
    n_old = x["n_old"]
    one, two = _bwd(case, X, xs, wsd, n_old, False), _bwd(case, X, xs, wsd, n_old, True)
    for o in ("dgi", "dgh", "dpre", "dagg", "dh0"):
        ratios[o] = _check("%s bwd %s" % (name, o), one[o], getattr(b64, o), b64.S[o], b64.n[o], dr.N0_STEP, dr.C_BOUND)
    for o in ("dgi", "dgh_n", "dpre", "dagg"):
        r = _check("%s bwd2 %s" % (name, o), two[o], getattr(b64, o), b64.S[o], b64.n[o], dr.N0_STEP, dr.C_BOUND)
        ratios[o] = max(ratios.get(o, 0.0), r)
    gp = two["grad_prev"]
    if x["prev_idx"] is not None and n_old == 0:
        assert torch.isnan(gp).all(), name + ": grad_prev written although no node is old"
    else:
        ratios["grad_prev"] = _check("%s bwd2 grad_prev" % name, gp, b64.grad_prev, b64.S["grad_prev"], b64.n["grad_prev"], dr.N0_STEP,
                                     dr.C_BOUND)
    # one kernel, two argument sets: the shared outputs agree bit for bit
    for o in ("dgi", "dpre", "dagg"):
        assert torch.equal(one[o], two[o]), "%s: %s differs between rg_dense_train_bwd and _bwd2" % (name, o)
    assert torch.equal(one["dgh"][:, 2 * d:], two["dgh_n"]) and torch.equal(one["dgh"][:, :2 * d], one["dgi"][:, :2 * d]), name + ": dgh blocks"
    if x["prev_idx"] is None:
        assert torch.equal(one["dh0"], gp), name + ": grad_prev != dh0 with prev_idx NULL"
    elif n_old:
        p_idx = X["prev_idx"].long()
        assert torch.equal(one["dh0"][p_idx >= 0], gp[p_idx[p_idx >= 0]]), name + ": grad_prev != dh0 gathered by prev_idx"
    # second run, through the engine wrappers
    mask = X["mask"]
    a1 = eng.dense_train_bwd(X["grad_hidden"], wsd, xs, mask, case.keep, act, X["W_h"], X["w_ih"], X["w_hh"])
    for t, o in zip(a1, ("dgi", "dgh", "dpre", "dagg", "dh0")):
        assert torch.equal(t, one[o]), "%s: second run of rg_dense_train_bwd differs in %s" % (name, o)
    if x["prev_idx"] is None or n_old:
        a2 = eng.dense_train_bwd2(X["grad_hidden"], wsd, xs, mask, case.keep, act, X["W_h"], X["w_ih"], X["w_hh"], X["prev_idx"],
                                  n if x["prev_idx"] is None else n_old)
        for t, o in zip(a2, ("dgi", "dgh_n", "dpre", "dagg", "grad_prev")):
            assert torch.equal(t, two[o]), "%s: second run of rg_dense_train_bwd2 differs in %s" % (name, o)
    return ratios


def _addmm_case(case):
    from red_gnn_amd import _lib, engine as eng
    L, p = _lib.lib(), _lib.ptr
    x = dr.inputs(case)
    base_buf, g, W = _dev(x["base"]), _dev(x["g"]), _dev(x["W"])
    ref = dr.rows_addmm(x["base"][:, :case.cols], x["g"], x["W"])

    def run():
        if case.alias:      # out = base: the sum lands in the base buffer's first `cols` columns, the rest of a spaced row stays
            buf = base_buf.clone()
            out, ldo = buf, case.base_width
        else:
            buf = base_buf
            out, ldo = _nan(case.n_rows, case.cols), case.cols
        _lib.check(L.rg_rows_addmm(p(buf), case.base_width, p(g), case.g_width, case.k, p(W), case.cols, case.n_rows, p(out), ldo,
                                   _lib.stream_ptr()))
        return out
    out = run()
    r = _check(case.name, out[:, :case.cols].contiguous(), ref.out, ref.S["out"], ref.n["out"], dr.N0_ROWS, dr.C_BOUND_ROWS)
    assert torch.equal(out[:, case.cols:], base_buf[:, case.cols:]) or not case.alias, case.name + ": columns beyond n were touched"
    assert torch.equal(run(), out), case.name + ": second run differs"
    if not case.alias:
        assert torch.equal(base_buf, _dev(x["base"])), case.name + ": base was modified"
        assert torch.equal(eng.rows_addmm(base_buf[:, :case.cols], g, W), out), case.name + ": engine.rows_addmm differs"
    return dict(out=r)


def _tables_case(case):
    from red_gnn_amd import _lib, engine as eng
    L, p = _lib.lib(), _lib.ptr
    x = dr.inputs(case)
    nl, rows, B, d, ld, ap = case.n_layer, case.n_rows, case.B, case.d, case.ld, case.ap
    dev = {k: [_dev(t) for t in x[k]] for k in ("rela", "Wr", "Wqr", "bqr")}
    q_rel = _dev(x["q_rel"], torch.int64)
    arr = lambda ts: (C.c_void_p * nl)(*[t.data_ptr() for t in ts])

    def run():
        a_r, a_q = _nan(nl, rows, ap), _nan(nl, B, ap)
        pad = _nan(nl, rows, ld) if ld != d else None
        _lib.check(L.rg_attn_tables(nl, rows, B, d, ld, case.attn_dim, ap, arr(dev["rela"]), arr(dev["Wr"]), arr(dev["Wqr"]), arr(dev["bqr"]),
                                    p(q_rel), p(a_r), p(a_q), p(pad), _lib.stream_ptr()))
        return a_r, a_q, pad
    a_r, a_q, pad = run()
    ratios = {}
    for l in range(nl):
        t = dr.attn_tables(x["rela"][l], x["Wr"][l], x["Wqr"][l], x["bqr"][l], x["q_rel"], ap, ld)
        for o, got in (("a_r", a_r[l]), ("a_q", a_q[l])):
            r = _check("%s layer %d %s" % (case.name, l, o), got, getattr(t, o), t.S[o], t.n[o], dr.N0_ROWS, dr.C_BOUND_ROWS)
            ratios[o] = max(ratios.get(o, 0.0), r)
            assert not got[:, case.attn_dim:].any(), "%s layer %d: pad columns of %s" % (case.name, l, o)
        if pad is not None:      # a bit copy with zero columns d .. ld - 1
            assert np.array_equal(pad[l].cpu().numpy(), t.rela_pad.astype(np.float32)), "%s layer %d: rela_pad" % (case.name, l)
    # queries that repeat a relation get the same row
    q = x["q_rel"]
    assert torch.equal(a_q[:, 1], a_q[:, 0]) and q[1] == q[0]
    again = run()
    assert torch.equal(again[0], a_r) and torch.equal(again[1], a_q) and (pad is None or torch.equal(again[2], pad)), case.name
    layers = [types.SimpleNamespace(rela_embed=types.SimpleNamespace(weight=dev["rela"][l]), Wr_attn=types.SimpleNamespace(weight=dev["Wr"][l]),
                                    Wqr_attn=types.SimpleNamespace(weight=dev["Wqr"][l], bias=dev["bqr"][l])) for l in range(nl)]
    for l, (e_r, e_q, e_p) in enumerate(eng.attn_tables(layers, q_rel, d, ld, case.attn_dim, ap)):
        assert torch.equal(e_r, a_r[l]) and torch.equal(e_q, a_q[l]) and torch.equal(e_p, pad[l] if pad is not None else dev["rela"][l])
    return ratios


@pytest.mark.parametrize("name", list(dr.CASES))
def test_dense_kernels_vs_reference(name):
    case = dr.CASES[name]
    ratios = {"step": _step_case, "addmm": _addmm_case, "tables": _tables_case}[case.kind](case)
    torch.cuda.synchronize()
    print("%s: %s" % (name, " ".join("%s=%.3g" % kv for kv in ratios.items())))


def test_argument_errors_are_reported():
    """Unsupported shapes return non-zero with the header's wording and launch nothing; the process stays usable (a supported call
    afterwards still meets the reference)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    buf = torch.zeros(64 * 1024, dtype=torch.float32, device="cuda")
    idx = torch.zeros(16, dtype=torch.int32, device="cuda")
    b, s = p(buf), _lib.stream_ptr()
    for d in (128, 12, 18):
        with pytest.raises(_lib.NativeError, match=r"rg_dense_train_bwd: hidden_dim %d not supported \(16\.\.64, multiple of 4\)" % d):
            _lib.check(L.rg_dense_train_bwd(16, d, b, b, b, None, 1.0, 1, b, b, b, b, b, b, b, b, s))
        with pytest.raises(_lib.NativeError, match=r"rg_dense_train_bwd2: hidden_dim %d not supported \(16\.\.64, multiple of 4\)" % d):
            _lib.check(L.rg_dense_train_bwd2(16, d, b, b, b, None, 1.0, 1, b, b, b, p(idx), b, b, b, b, b, s))
    with pytest.raises(_lib.NativeError, match=r"rg_dense_train_fwd_as: Ws_next needs a_s_out, 1 <= attn_dim <= 16 .*attn_dim=17 ap=20"):
        _lib.check(L.rg_dense_train_fwd_as(16, 64, b, b, p(idx), b, 1, b, b, b, b, None, b, 17, 20, b, b, b, b, s))
    with pytest.raises(_lib.NativeError, match=r"rg_dense_train_fwd: hidden_dim 18 not supported \(16\.\.64 in steps of 4, or 128\)"):
        _lib.check(L.rg_dense_train_fwd(16, 18, b, b, p(idx), b, 1, b, b, b, b, None, b, b, b, s))
    with pytest.raises(_lib.NativeError, match=r"rg_rows_addmm: k=5 \(1\.\.32\) n=18 \(4\.\.128, multiple of 4\)"):
        _lib.check(L.rg_rows_addmm(b, 20, b, 8, 5, b, 18, 16, b, 20, s))
    with pytest.raises(_lib.NativeError, match=r"rg_rows_addmm: k=33 \(1\.\.32\) n=64"):
        _lib.check(L.rg_rows_addmm(b, 64, b, 36, 33, b, 64, 16, b, 64, s))
    torch.cuda.synchronize()
    assert not buf.any()
    for name in ("n17", "am48_k5_alias"):
        case = dr.CASES[name]
        {"step": _step_case, "addmm": _addmm_case}[case.kind](case)
    torch.cuda.synchronize()
