"""The six fused inference dense kernels - rg_dense_fwd / rg_dense_fwd_dev at precision 0 (f32 MFMA: dense.hip, dense128.hip), 1 (two-term
f16 split: dense_split.hip, dense128_split.hip) and 2 (exact three-term split, the model's default: dense_split3.hip,
dense128_split3.hip) - called directly, against the fp64 reference of tests/dense_ref.py over its inference table (INFER_CASES: one case
per dispatch condition; each ``why`` cites the line it flips).  hidden_out, a_s_out and scores_all carry 32 guard rows / entries and are
pre-filled with NaN.  After the call every row < n is fully written and every element - pad columns included, nothing exempt - satisfies

    precision 0, 2    |gpu - ref64| <= C_BOUND (n + n0) u S + 1e-30                          (C_BOUND = 4 x 0.3, as the training kernels)
    precision 1       |gpu - ref64| <= C_BOUND (n + n0) u S + C2 p 2^-22 S + 1e-30           (C2 = 2 x 0.125: dense_ref.C2_F16X2)

(dense_ref's docstring defines S, n, n0; p = matrix products chained into the element: 2 for the state, 3 for a_s and the score;
tests/test_dense_ref.py keeps both constants honest on the CPU and shows that the bounds reject four injected faults).  a_s columns
attn_dim .. ap - 1 and hidden_out columns d .. ld - 1 are exactly 0; scores_all holds a bounded value at every nodes entry and its NaN
bit pattern everywhere else; guard rows are untouched.  Calls of one case agree bit for bit: a second run, the scores without
hidden_out, the state without the projections, and rg_dense_fwd_dev whatever its n_hint.  One test holds the projection products
(Ws_next, W_final) bit for bit through the public entry at every width, d = 128 included.

The kernels' own worst ratios |gpu - ref64| / ((n + n0) u S) per case are printed under -s and summarised in KERNEL_RATIOS below
(information only - the assertions use the bounds above).
"""
import functools

import numpy as np
import pytest
import torch

from tests import dense_ref as dr

pytestmark = pytest.mark.gpu

# the kernels' worst |gpu - ref64| / ((n + n0) u S) per precision and output over the whole table, as measured on an MI355X (information
# only; allowed: 1.2, at precision 1 plus its 2^-22 term).  The worst case of every entry is w_d1_ld4, where n + n0 = 17 is smallest;
# over the cases with d >= 20 the worst is spike_d20_ld32: hidden 0.036 / 0.045 / 0.045, a_s 0.013 / 0.014 / 0.008, score 0.007 / 0.012 /
# 0.009 at precisions 0 / 1 / 2
KERNEL_RATIOS = {
    0: {"hidden": 0.044, "a_s": 0.043, "score": 0.051},
    1: {"hidden": 0.072, "a_s": 0.087, "score": 0.081},
    2: {"hidden": 0.084, "a_s": 0.086, "score": 0.082},
}
# wall time of this file on an MI355X (information only): 4.0 s (183 tests; the slowest, n32769_d128 at precision 0, 0.5 s)

GUARD = 32
NAN = float("nan")
NAN_BITS = int(np.array([NAN], np.float32).view(np.int32)[0])
PRECISION_NAMES = {0: "f32", 1: "f16x2", 2: "f16x3"}
_PARAMS = [pytest.param(c.name, p, id="%s-%s" % (c.name, PRECISION_NAMES[p])) for c in dr.INFER_CASES.values() for p in c.precisions]


def _nan(*shape):
    t = torch.full(shape, NAN, dtype=torch.float32, device="cuda")
    assert int(t.view(torch.int32).flatten()[0]) == NAN_BITS
    return t


def _untouched(t):
    """Every element still holds the prefill's NaN bit pattern."""
    return bool((t.view(torch.int32) == NAN_BITS).all())


def _pad(a, rows, ld, fill=0.0):
    """[rows, ld] float32 device copy of a [r, d] array: pad columns zero, rows beyond r filled with ``fill``."""
    out = np.full((rows, ld), fill, np.float32)
    out[:, a.shape[1]:] = 0.0
    out[:a.shape[0], :a.shape[1]] = a
    return torch.as_tensor(out).cuda()


@functools.lru_cache(maxsize=2)
def _case(name):
    """(case, host inputs, fp64 reference, device inputs) - computed once per case, shared by its precisions."""
    case = dr.INFER_CASES[name]
    x = dr.infer_inputs(case)
    dev = lambda a, dt=torch.float32: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dt).cuda()
    X = {k: dev(x[k]) for k in ("W_h", "w_ih", "w_hh", "b_ih", "b_hh", "Ws_next", "W_final")}
    X["agg"] = _pad(x["agg"], case.n, case.ld)
    X["hidden_prev"] = None if x["hidden_prev"] is None else _pad(x["hidden_prev"], x["hidden_prev"].shape[0], case.ld)
    X["prev_idx"] = dev(x["prev_idx"], torch.int32)
    X["nodes"] = dev(x["nodes"], torch.int32)
    return case, x, dr.infer_forward(case, x), X


def _call(case, x, X, precision, ws=True, final=True, hidden=True, n=None, n_dev=None, n_hint=0):
    """One rg_dense_fwd (or, with n_dev, rg_dense_fwd_dev on buffers of capacity ``n``) into NaN-filled outputs with GUARD rows / entries
    to spare: (hidden_out or None, a_s_out or None, scores_all or None)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n = case.n if n is None else n
    ws, final = ws and X["Ws_next"] is not None, final and X["W_final"] is not None
    h_out = _nan(n + GUARD, case.ld) if hidden else None
    a_s = _nan(n + GUARD, case.ap) if ws else None
    scores = _nan(x["n_scores"] + GUARD) if final else None
    nb = int(L.rg_dense_scratch_bytes(case.d, precision))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    tail = (case.d, case.ld, p(X["agg"]), p(X["hidden_prev"]), p(X["prev_idx"]), p(X["W_h"]), case.act, p(X["w_ih"]), p(X["w_hh"]),
            p(X["b_ih"]), p(X["b_hh"]), p(X["Ws_next"]) if ws else None, case.attn_dim if ws else 0, case.ap if ws else 0, p(a_s),
            p(X["W_final"]) if final else None, p(X["nodes"]) if final else None, x["n_ent"] if final else 0, p(scores), p(h_out),
            precision, p(scratch), nb, _lib.stream_ptr())
    if n_dev is None:
        _lib.check(L.rg_dense_fwd(n, *tail))
    else:
        _lib.check(L.rg_dense_fwd_dev(n, p(n_dev), n_hint, *tail))
    torch.cuda.synchronize()
    return h_out, a_s, scores


def _check(what, gpu, ref, S, n, out, precision):
    """Every element of ``gpu`` (a numpy array) written and within the precision's bound of ``ref``.  Returns the worst ratio
    |gpu - ref| / ((n + n0) u S)."""
    gpu = np.asarray(gpu, np.float64).reshape(np.shape(ref))
    assert not np.isnan(gpu).any(), "%s: %d elements were never written (or are NaN)" % (what, int(np.isnan(gpu).sum()))
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    ok = np.abs(gpu - ref) <= dr.infer_bound(precision, S, n, out)
    ratio = dr.worst_ratio(gpu, ref, S, n, dr.N0_STEP)
    assert ok.all(), ("%s: %d of %d elements beyond the bound; worst ratio %.3g; first at %s: gpu %.9g ref %.9g S %.3g n %d"
                      % (what, int((~ok).sum()), ok.size, ratio, np.argwhere(~ok)[0], gpu[~ok][0], ref[~ok][0], S[~ok][0], int(n)))
    return ratio


def _check_outputs(what, case, x, f64, precision, h_out, a_s, scores):
    """The contract of one call's outputs; returns the worst ratios per output."""
    n, d, ld = case.n, case.d, case.ld
    ratios = {}
    if h_out is not None:
        h = h_out.cpu().numpy()
        ratios["hidden"] = _check(what + " hidden", h[:n, :d], f64.hidden, f64.S["hidden"], f64.n["hidden"], "hidden", precision)
        # zero pad columns in agg and hidden_prev, zero padded weights and biases: 0.5 tanh(0) + 0.5 h0_pad = 0 exactly
        assert not h[:n, d:].any() and not np.isnan(h[:n, d:]).any(), what + ": pad columns d .. ld - 1 of hidden_out are not exactly 0"
        assert _untouched(h_out[n:]), what + ": guard rows of hidden_out written"
    if a_s is not None:
        a = a_s.cpu().numpy()
        ratios["a_s"] = _check(what + " a_s", a[:n], f64.a_s, f64.S["a_s"], f64.n["a_s"], "a_s", precision)
        assert not a[:n, case.attn_dim:].any(), what + ": pad columns attn_dim .. ap - 1 of a_s are not exactly 0"
        assert _untouched(a_s[n:]), what + ": guard rows of a_s_out written"
    if scores is not None:
        s = scores.cpu().numpy()
        at = x["nodes"][:, 0].astype(np.int64) * x["n_ent"] + x["nodes"][:, 1]
        ratios["score"] = _check(what + " score", s[at], f64.score, f64.S["score"], f64.n["score"], "score", precision)
        rest = np.ones(len(s), bool)
        rest[at] = False
        assert (s.view(np.int32)[rest] == NAN_BITS).all(), what + ": scores_all written outside the nodes' entries"
    return ratios


@pytest.mark.parametrize("name,precision", _PARAMS)
def test_dense_fwd_vs_reference(name, precision):
    case, x, f64, X = _case(name)
    what = "%s %s" % (name, PRECISION_NAMES[precision])
    h_out, a_s, scores = _call(case, x, X, precision, hidden=not case.no_hidden)
    ratios = _check_outputs(what, case, x, f64, precision, h_out, a_s, scores)
    eq = lambda a, b: (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a second run is the first, bit for bit
    h2, a2, s2 = _call(case, x, X, precision, hidden=not case.no_hidden)
    assert eq(h2, h_out) and eq(a2, a_s) and eq(s2, scores), what + ": second run differs"
    if case.no_hidden:
        # hidden_out = NULL: the scores are those of the call with hidden_out, whose state is checked here
        h3, _, s3 = _call(case, x, X, precision)
        ratios.update(_check_outputs(what + " (with hidden_out)", case, x, f64, precision, h3, None, s3))
        assert eq(s3, scores), what + ": scores differ without hidden_out"
    elif case.attn_dim or case.readout:
        # the state does not depend on which projection the launch carries
        h3, _, _ = _call(case, x, X, precision, ws=False, final=False)
        assert eq(h3, h_out), what + ": the state differs from that of the call with neither projection"
        if case.attn_dim and case.readout:
            _, a4, _ = _call(case, x, X, precision, final=False)
            assert eq(a4, a_s), what + ": a_s differs without the readout"
    print("%s: %s" % (what, " ".join("%s=%.3g" % kv for kv in ratios.items())))


@pytest.mark.parametrize("precision", [0, 1, 2], ids=list(PRECISION_NAMES.values()))
@pytest.mark.parametrize("name", ["w_d64", "w_d20_ld32", "w_d128"])
def test_dense_fwd_dev_equals_dense_fwd(name, precision):
    """rg_dense_fwd_dev on buffers of capacity n + 300 with the row count on the device: rows < n are rg_dense_fwd's bit for bit whatever
    n_hint says (it only sizes the grid, dense_common.h:67 dense_grid; a 16-row tile is computed by one wave whatever the grid), rows
    beyond n keep their sentinel."""
    case, x, _, X = _case(name)
    n, cap = case.n, case.n + 300
    rng = np.random.default_rng(7)
    want = _call(case, x, X, precision)
    Xc = dict(X)
    # rows n .. cap - 1 exist and hold finite numbers; their (query, entity) pairs point into the guard entries of scores_all
    Xc["agg"] = _pad(x["agg"], cap, case.ld, fill=3.0)
    prev = np.full(cap, -1, np.int32)
    if x["prev_idx"] is not None:
        prev[:n] = x["prev_idx"]
        prev[n:] = rng.integers(0, max(x["n_old"], 1), cap - n) if x["n_old"] else -1
        Xc["prev_idx"] = torch.as_tensor(prev).cuda()
    flat = np.r_[x["nodes"][:, 0].astype(np.int64) * x["n_ent"] + x["nodes"][:, 1], x["n_scores"] + np.arange(cap - n) % GUARD]
    Xc["nodes"] = torch.as_tensor(np.stack([flat // x["n_ent"], flat % x["n_ent"]], 1).astype(np.int32)).cuda()
    n_dev = torch.tensor([n], dtype=torch.int32, device="cuda")
    for n_hint in (0, n // 7, n):
        got = _call(case, x, Xc, precision, n=cap, n_dev=n_dev, n_hint=n_hint)
        for o, g, w in zip(("hidden", "a_s"), got, want):
            assert torch.equal(g[:n].view(torch.int32), w[:n].view(torch.int32)), "%s n_hint=%d: %s differs from rg_dense_fwd" % (name, n_hint, o)
            assert _untouched(g[n:]), "%s n_hint=%d: %s written beyond row n" % (name, n_hint, o)
        assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), "%s n_hint=%d: scores differ from rg_dense_fwd" % (name, n_hint)


@pytest.mark.parametrize("precision", [0, 1, 2], ids=list(PRECISION_NAMES.values()))
@pytest.mark.parametrize("d", [3, 20, 32, 33, 48, 63, 64, 128])
def test_projection_products_on_one_hot_states(d, precision):
    """The products with Ws_next and W_final through the public entry.  All of W_h, weight_ih, weight_hh and the biases are zero except
    b_iz = 30: z = rcp(1 + exp(-30)) = 1.0f exactly, n = tanh(0) = 0, and the new state is h0 in every one of the six forms of the state
    update.  With h0 = one-hot rows times powers of two (the hot column cycling over all d) and weights with all 24 mantissa bits in use,
    a_s[:, e] = Ws[e, k] 2^j and score = W_final[k] 2^j are single products without a sum: at precisions 0 and 2 they must come out BIT
    FOR BIT - a missing partial product of a three-term kernel (an error of order 4 u) fails here and under no S-bound; at precision 1
    within 2^-21 relative (two operands of 22 bits)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    rng = np.random.default_rng(80 + d)
    n, ld, attn, n_ent = 4 * d + 37, (d + 3) // 4 * 4, 16, 37

    def full24(*shape):        # fp32 values with random 24-bit mantissas (last bit set), random signs, five binades
        m = (rng.integers(1 << 23, 1 << 24, shape) | 1).astype(np.float64) * 2.0 ** -24
        return (m * rng.choice([-1.0, 1.0], shape) * 2.0 ** rng.integers(-4, 1, shape)).astype(np.float32)

    Ws, W_final = full24(attn, d), full24(d)
    assert np.array_equal(Ws.astype(np.float64), Ws) and (Ws.view(np.int32) & 1).all()
    k, pw = np.arange(n) % d, 2.0 ** (np.arange(n) % 7 - 6.0)
    h0 = np.zeros((n, d), np.float32)
    h0[np.arange(n), k] = pw
    prev = rng.permutation(n).astype(np.int32)
    hprev = np.zeros((n, d), np.float32)
    hprev[prev] = h0
    b_ih = np.zeros(3 * d, np.float32)
    b_ih[d:2 * d] = 30.0
    dev = lambda a: torch.as_tensor(a).cuda()
    zeros = lambda *s: torch.zeros(*s, dtype=torch.float32, device="cuda")
    agg, hp = _pad(rng.standard_normal((n, d)).astype(np.float32), n, ld), _pad(hprev, n, ld)
    flat = np.sort(rng.choice(3 * n, n, replace=False))
    nodes = dev(np.stack([flat // n_ent, flat % n_ent], 1).astype(np.int32))
    h_out, a_s, scores = _nan(n + GUARD, ld), _nan(n + GUARD, attn), _nan(3 * n + GUARD)
    nb = int(L.rg_dense_scratch_bytes(d, precision))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    # (every operand in a variable of its own that outlives the call: the pointer of a temporary would be one into freed memory)
    prev_d, W_h, w_ih, w_hh, b_ih_d, b_hh = dev(prev), zeros(d, d), zeros(3 * d, d), zeros(3 * d, d), dev(b_ih), zeros(3 * d)
    Ws_d, W_final_d = dev(Ws), dev(W_final)
    _lib.check(L.rg_dense_fwd(n, d, ld, p(agg), p(hp), p(prev_d), p(W_h), 0, p(w_ih), p(w_hh), p(b_ih_d), p(b_hh), p(Ws_d), attn, attn, p(a_s),
                              p(W_final_d), p(nodes), n_ent, p(scores), p(h_out), precision, p(scratch), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    del prev_d, W_h, w_ih, w_hh, b_ih_d, b_hh, Ws_d, W_final_d
    h, a, s = h_out.cpu().numpy(), a_s.cpu().numpy(), scores.cpu().numpy()
    assert _untouched(h_out[n:]) and _untouched(a_s[n:])
    want_h = np.zeros((n, ld), np.float32)
    want_h[:, :d] = h0
    assert np.array_equal(h[:n].view(np.int32), want_h.view(np.int32)), "the new state is not h0 bit for bit"
    want_a = (Ws.T[k].astype(np.float64) * pw[:, None]).astype(np.float32)
    want_s = (W_final[k].astype(np.float64) * pw).astype(np.float32)
    assert np.array_equal(want_a.astype(np.float64), Ws.T[k].astype(np.float64) * pw[:, None])      # a power of two: no rounding
    got_s = s[flat]
    rest = np.ones(len(s), bool)
    rest[flat] = False
    assert (s.view(np.int32)[rest] == NAN_BITS).all()
    if precision == 1:
        assert (np.abs(a[:n].astype(np.float64) - want_a) <= 2.0 ** -21 * np.abs(want_a)).all()
        assert (np.abs(got_s.astype(np.float64) - want_s) <= 2.0 ** -21 * np.abs(want_s)).all()
    else:
        bad = np.argwhere(a[:n].view(np.int32) != want_a.view(np.int32))
        assert not len(bad), "a_s differs from Ws[e, k] 2^j in %d of %d elements; first at %s: %r != %r" % (
            len(bad), want_a.size, bad[0], a[tuple(bad[0])], want_a[tuple(bad[0])])
        assert np.array_equal(got_s.view(np.int32), want_s.view(np.int32)), "the scores differ from W_final[k] 2^j"
