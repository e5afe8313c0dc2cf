"""Plain-numpy reference of the DENSE half of a training step (what include/redgnn.h promises for rg_dense_train_fwd / _fwd_as,
rg_dense_train_bwd / _bwd2, rg_rows_addmm and rg_attn_tables), plus the case table the dense-kernel tests share.  TEST INFRASTRUCTURE.

    forward    h0 = hidden_prev[prev_idx] (0 where prev_idx = -1 or NULL)
               pre = agg W_h^T;  x = act(pre) * mask                                      (act: 0 identity, 1 relu, 2 tanh)
               r = sigmoid(W_ir x + b_ir + W_hr h0 + b_hr);  z = sigmoid(W_iz x + b_iz + W_hz h0 + b_hz)
               hn = W_hn h0 + b_hn;  n = tanh(W_in x + b_in + r hn);  hidden = (1 - z) n + z h0;  a_s = hidden Ws_next^T
               workspace ws [rows, 5, d] = {r, z, n, h0, hn}
               score = hidden . W_final, scattered to scores_all[nodes[:, 0] * n_ent + nodes[:, 1]]   (inference: rg_dense_fwd; its
               contract, its case table and precision 1's two-term emulation are at the end of the file)
    backward   from g = grad_hidden and the SAVED ws / x (inputs, exactly as the kernels take them):
               dn = g (1 - z) (1 - n^2);  dr = dn hn r (1 - r);  dz = g (h0 - n) z (1 - z)
               dgi = (dr, dz, dn);  dgh = (dr, dz, dn r);  dgh_n = dn r
               dx = dgi W_ih;  dh0 = g z + dgh W_hh;  dpre = dx * mask * act'(.);  dagg = dpre W_h
                   act' : 1 | 1[x > 0] | 1 - y^2 with y = x * keep under a mask (x = tanh(pre) / keep where kept), y = x without
               grad_prev[prev_idx[m]] = dh0[m] for prev_idx[m] >= 0  (prev_idx NULL: grad_prev = dh0)
               weight gradients (``backward`` given agg; what models._DenseStep.backward returns besides dagg and grad_prev):
               grad_W_h = dpre^T agg;  grad_w_ih = dgi^T x;  grad_w_hh = dgh^T h0;  grad_b_ih = dgi.sum(0);  grad_b_hh = dgh.sum(0)
               with Ws_next: grad_Ws = g_as[:, :a]^T hidden, and g above = grad_hidden + g_as[:, :a] Ws_next (returned as grad_hidden)
    rows_addmm out = base + g[:, :k] W          attn_tables a_r = rela Wr^T, a_q = rela[q_rel] Wqr^T + bqr, rela padded to ld columns

Every function takes ``dtype``: np.float64 is the reference; np.float32 (the same code, the same order) is the yardstick of what a
correct fp32 evaluation costs.  Besides each output the functions return, in fp64, ``n`` = the number of terms summed into the
element along its longest chain of dot products (a product over inputs that are themselves sums adds their count), and ``S`` = the
same expression with every term replaced by its absolute value: |agg| |W_h|^T for pre, |1| + |z| for 1 - z, 1 + n^2 for 1 - n^2,
|h0| + |n| for h0 - n.  Through a function the pre-activation's S is carried to first order, plus the function's own rounding:

    relu, identity   S        (1-Lipschitz: a sign flip of a pre-activation within its error moves x by no more than that error,
                               so no element at the kink needs exempting)
    f = sigmoid      |f'| (S + 1) + |f|     f' = f (1 - f)      the + 1: the exp's own 1-ulp relative error moves f by |f'| u
    f = tanh         |f'| (S + 1) + |f|     f' = 1 - f^2
    a product        S_a |b| + |a| S_b      (r hn, (1 - z) n, z h0 with h0 exact: S_z |h0|)

The error of an fp32 evaluation scales with u * S:

    |fp32 - fp64| <= c * (n + n0) * u * S + tiny         u = 2^-24, tiny = 1e-30 (S = 0: the value must be exactly 0)

n0 (``N0_STEP`` = 12) is the elementwise work between the sums of the step that n does not count: activation (exp, reciprocal, the
1 - e and the product: 4), mask, the bias adds (2), the product and the add of r hn (2), the three operations of the state update:
12.  The two row-wise products have n0 = 1 (the final add).  ``C_BOUND`` / ``C_BOUND_ROWS`` below are 4 x the worst ratio
|ref32 - ref64| / ((n + n0) u S) measured over every element of every output of every case of the table (test_dense_ref.py keeps
that measurement honest: it fails if a case exceeds REF32_WORST_RATIO / REF32_WORST_RATIO_ROWS).

The weight gradients are sums over the node rows.  Their fp32 evaluation sums in the shape of rg_gram_tn (tests/gram_ref.py: waves of
rows_per_wave rows, four chains of 256 partials), their n is the n of the summed quantity (3 d for dpre, 0 for dgi / dgh; a + 1 more
throughout when g itself is the sum grad_hidden + g_as Ws_next) plus the longest chain of that shape (gram_ref.n_terms: rows_per_wave
+ 256 + 3 for a product, 4 more for a column sum), and their S is the same product over the S of the summed quantity.  The same n
serves the routes that form these sums with a library GEMM (fewer than 32768 rows, d = 128).  ``REF32_WORST_RATIO_WGRAD`` /
``C_BOUND_WGRAD`` are their own constants, measured over ROUTE_CASES.
"""
import types

import numpy as np

U = 2.0 ** -24
TINY = 1e-30
# measured: max over all cases, outputs and elements of |ref32 - ref64| / ((n + n0) * u * S), rounded up
# (test_fp32_reference_within_its_bound prints the per-case figures).  Two constants because the two accountings differ in kind: the
# step's n counts whole dot-product chains (its worst element, a dgi entry - five products in a row, n = 0 - reaches 0.274), the
# row-wise products count every single rounding (k = 1: two roundings against n + n0 = 3, 0.561)
REF32_WORST_RATIO = 0.3
REF32_WORST_RATIO_ROWS = 0.6
# the GPU's allowance: 4 x the fp32 reference's own cost (another summation order in the MFMA chains, fused multiply-adds, the 1-ulp
# hardware exp / reciprocal); the factor tests/_util.assert_close_fp32 and layer_ref.C_BOUND grant the GPU over the CPU fp32 path
C_BOUND = 4.0 * REF32_WORST_RATIO
C_BOUND_ROWS = 4.0 * REF32_WORST_RATIO_ROWS
N0_STEP = 12
N0_ROWS = 1
# measured: max over ROUTE_CASES, the WGRAD_OUTPUTS and their elements of |ref32 - ref64| / ((n + n0) u S), rounded up
# (test_dense_ref.py::test_fp32_weight_gradients_within_their_bound prints the per-case figures; the worst: bwd2_d64_as16's grad_Ws
# 0.00047, aten_d128's grad_w_ih 0.00040).  Three orders below REF32_WORST_RATIO: over a chain of ~355 additions the roundings mostly
# cancel, where a dgi entry is five products in a row against n = 0
REF32_WORST_RATIO_WGRAD = 0.0005
C_BOUND_WGRAD = 4.0 * REF32_WORST_RATIO_WGRAD

ACT = {"idd": 0, "relu": 1, "tanh": 2}
FWD_OUTPUTS = ("hidden", "x", "ws", "a_s")
BWD_OUTPUTS = ("dgi", "dgh", "dgh_n", "dpre", "dagg", "dh0", "grad_prev")
WGRAD_OUTPUTS = ("grad_W_h", "grad_w_ih", "grad_w_hh", "grad_b_ih", "grad_b_hh", "grad_Ws")


def bound(S, n, n0, c):
    return c * (np.asarray(n, np.float64) + n0) * U * np.asarray(S, np.float64) + TINY


def worst_ratio(val, ref, S, n, n0):
    """max (|val - ref| - tiny) / ((n + n0) u S) over the elements: the c that ``bound`` would need (inf where S = 0 and the values
    differ by more than tiny)."""
    err = np.maximum(np.abs(np.asarray(val, np.float64) - np.asarray(ref, np.float64)) - TINY, 0.0)
    den = (np.asarray(n, np.float64) + n0) * U * np.asarray(S, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, err / den, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


def _c(dt, x):
    return None if x is None else np.asarray(x).astype(dt)


def _sigmoid(x):
    one = x.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-x))


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def _gather(hidden_prev, prev_idx, n, d, dt):
    h0 = np.zeros((n, d), dt)
    if prev_idx is not None:
        old = np.asarray(prev_idx) >= 0
        h0[old] = hidden_prev[np.asarray(prev_idx, np.int64)[old]]
    return h0


def _stale_all_new(h0, prev_idx):
    """fault: a 16-row tile without an old row keeps the h0 of the last tile that had one (negative tests only)."""
    if prev_idx is None:
        return h0
    old, last, h0 = np.asarray(prev_idx) >= 0, None, h0.copy()
    for t in range(0, len(h0), 16):
        if old[t:t + 16].any():
            last = h0[t:t + 16].copy()
        elif last is not None:
            h0[t:t + 16] = last[:len(h0[t:t + 16])]
    return h0


def _fwd_values(dt, agg, hidden_prev, prev_idx, W_h, act, w_ih, w_hh, b_ih, b_hh, mask, Ws_next, W_final=None, fault=None):
    agg, hidden_prev, W_h, w_ih, w_hh, b_ih, b_hh, mask, Ws_next, W_final = (_c(dt, t) for t in (agg, hidden_prev, W_h, w_ih, w_hh, b_ih, b_hh,
                                                                                                mask, Ws_next, W_final))
    n, d = agg.shape
    one = dt.type(1)
    h0 = _gather(hidden_prev, prev_idx, n, d, dt)
    if fault == "stale_all_new":
        h0 = _stale_all_new(h0, prev_idx)
    pre = agg @ W_h.T
    a = pre if act == 0 else np.maximum(pre, dt.type(0)) if act == 1 else np.tanh(pre)
    x = a if mask is None else a * mask
    gi = x @ w_ih.T + b_ih
    hh = h0 @ w_hh.T
    b_hn = b_hh[2 * d:] if fault != "no_b_hn" else np.zeros(d, dt)      # fault: one gate bias dropped (negative tests only)
    r = _sigmoid(gi[:, :d] + hh[:, :d] + b_hh[:d])
    z = _sigmoid(gi[:, d:2 * d] + hh[:, d:2 * d] + b_hh[d:2 * d])
    hn = hh[:, 2 * d:] + b_hn
    npre = gi[:, 2 * d:] + r * hn
    ng = np.tanh(npre)
    hidden = (one - z) * ng + z * h0
    a_s = None if Ws_next is None else hidden @ Ws_next.T
    # fault: the readout reads the old state instead of the new one (negative tests only)
    score = None if W_final is None else (h0 if fault == "readout_h0" else hidden) @ W_final
    return dict(h0=h0, pre=pre, a=a, x=x, r=r, z=z, hn=hn, ng=ng, hidden=hidden, a_s=a_s, score=score)


def forward(agg, hidden_prev, prev_idx, W_h, act, w_ih, w_hh, b_ih, b_hh, mask=None, Ws_next=None, ap=None, dtype=np.float64, fault=None,
            W_final=None):
    """hidden [n, d], x [n, d], ws [n, 5, d] = {r, z, n, h0, hn}, a_s [n, ap] (None without Ws_next; columns attn_dim .. ap - 1 zero),
    score [n] = hidden . W_final (None without W_final: the readout of rg_dense_fwd, before its scatter) in ``dtype``; .S / .n per output
    name in fp64 (include/redgnn.h, rg_dense_train_fwd / rg_dense_train_fwd_as / rg_dense_fwd)."""
    act = ACT.get(act, act)
    args = (agg, hidden_prev, prev_idx, W_h, act, w_ih, w_hh, b_ih, b_hh, mask, Ws_next, W_final)
    v = _fwd_values(np.dtype(dtype), *args, fault=fault)
    w = _fwd_values(np.dtype(np.float64), *args)
    A = lambda t: np.abs(np.asarray(t, np.float64))
    n_rows, d = np.shape(agg)
    S_pre = A(agg) @ A(W_h).T
    S_a = S_pre if act != 2 else (1 - w["a"] ** 2) * (S_pre + 1) + np.abs(w["a"])
    S_x = S_a if mask is None else S_a * A(mask)
    Wi, Wh, bi, bh, h0 = A(w_ih), A(w_hh), A(b_ih), A(b_hh), np.abs(w["h0"])
    gate = lambda g: S_x @ Wi[g * d:(g + 1) * d].T + bi[g * d:(g + 1) * d]
    hside = lambda g: h0 @ Wh[g * d:(g + 1) * d].T + bh[g * d:(g + 1) * d]
    sig = lambda f, S: f * (1 - f) * (S + 1) + f
    S_r, S_z = sig(w["r"], gate(0) + hside(0)), sig(w["z"], gate(1) + hside(1))
    S_hn = hside(2)
    S_npre = gate(2) + S_r * np.abs(w["hn"]) + w["r"] * S_hn
    S_n = (1 - w["ng"] ** 2) * (S_npre + 1) + np.abs(w["ng"])
    S_h = S_z * (np.abs(w["ng"]) + h0) + (1 - w["z"]) * S_n
    n_x, n_rz, n_hn, n_n = d, 2 * d + 2, d + 1, 2 * d + 3
    S = dict(x=S_x, hidden=S_h, ws=np.stack([S_r, S_z, S_n, h0, S_hn], 1))
    n = dict(x=n_x, hidden=n_n, ws=np.array([n_rz, n_rz, n_n, 0, n_hn], np.float64).reshape(1, 5, 1))
    a_s = None
    if Ws_next is not None:
        attn = np.shape(Ws_next)[0]
        ap = (attn + 3) // 4 * 4 if ap is None else ap
        a_s = np.zeros((n_rows, ap), v["a_s"].dtype)
        a_s[:, :attn] = v["a_s"]
        S["a_s"] = np.zeros((n_rows, ap))
        S["a_s"][:, :attn] = S_h @ A(Ws_next).T
        n["a_s"] = n_n + d
    if W_final is not None:
        S["score"] = S_h @ A(W_final)
        n["score"] = n_n + d
    ws = np.stack([v["r"], v["z"], v["ng"], v["h0"], v["hn"]], 1)
    return types.SimpleNamespace(hidden=v["hidden"], x=v["x"], ws=ws, a_s=a_s, score=v["score"], S=S, n=n)


def scatter_scores(score, nodes, n_ent, size, fill=np.nan):
    """scores_all [size] as rg_dense_fwd leaves it: ``score`` at nodes[:, 0] * n_ent + nodes[:, 1], ``fill`` everywhere else."""
    out = np.full(size, fill, np.asarray(score).dtype)
    nodes = np.asarray(nodes, np.int64)
    out[nodes[:, 0] * n_ent + nodes[:, 1]] = score
    return out


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def _bwd_values(dt, g, ws, x, mask, keep, act, W_h, w_ih, w_hh, absolute, fault=None):
    """dgi, dgh, dpre, dagg, dh0; absolute = the S form (every term replaced by its absolute value, 1 - t by 1 + |t|)."""
    g, ws, x, mask, W_h, w_ih, w_hh = (_c(dt, t) for t in (g, ws, x, mask, W_h, w_ih, w_hh))
    n, d = x.shape
    ws = ws.reshape(n, 5, d)
    r, z, ng, h0, hn = (ws[:, i] for i in range(5))
    if fault == "col_shift":      # fault: the last, partly filled 16-column block reads z one column to the right (negative tests only)
        flat = ws.reshape(n, 5 * d)
        z = np.concatenate([z[:, :32], flat[:, d + 33:2 * d + 1]], 1)
    one = dt.type(1)
    if absolute:
        g, r, z, ng, h0, hn, W_h, w_ih, w_hh = (np.abs(t) for t in (g, r, z, ng, h0, hn, W_h, w_ih, w_hh))
        mask = None if mask is None else np.abs(mask)
        om = lambda t: one + t
        diff = h0 + ng
    else:
        om = lambda t: one - t
        diff = h0 - ng
    dn = g * om(z) * om(ng * ng)
    dr = dn * hn * r * om(r)
    dz = g * diff * z * om(z)
    dnr = dn * r if fault != "dgh_n_no_r" else dn      # fault: dgh's n block missing its * r (negative tests only)
    dgi, dgh = np.concatenate([dr, dz, dn], 1), np.concatenate([dr, dz, dnr], 1)
    dx = dgi @ w_ih
    dh0 = g * z + dgh @ w_hh
    v = dx if mask is None else dx * mask
    if act == 1:
        v = np.where(x > 0, v, dt.type(0))
    elif act == 2:
        y = x if mask is None else x * dt.type(keep)
        v = v * om(y * y)
    dagg = v @ W_h
    return dict(dgi=dgi, dgh=dgh, dgh_n=dnr, dpre=v, dagg=dagg, dh0=dh0)


def _scatter_prev(dh0, prev_idx, n_old):
    if prev_idx is None:
        return dh0
    out = np.zeros((n_old, dh0.shape[1]), dh0.dtype)
    p = np.asarray(prev_idx, np.int64)
    out[p[p >= 0]] = dh0[p >= 0]
    return out


def _cat_order(t, d):
    """fault: the hidden-side blocks assembled as (n, r, z) instead of (r, z, n) (negative tests only)."""
    return np.concatenate([t[2 * d:], t[:2 * d]], 0)


def backward(grad_hidden, ws, x, mask, keep, act, W_h, w_ih, w_hh, prev_idx=None, n_old=0, dtype=np.float64, fault=None, agg=None,
             g_as=None, Ws_next=None, hidden=None):
    """dgi, dgh [n, 3d], dgh_n, dpre, dagg, dh0 [n, d], grad_prev [n_old, d] (prev_idx NULL: = dh0) in ``dtype``; .S / .n per output name
    (include/redgnn.h, rg_dense_train_bwd / rg_dense_train_bwd2).  ws / x are the SAVED forward outputs, taken as given.
    With ``agg`` also the weight gradients grad_W_h [d, d], grad_w_ih, grad_w_hh [3d, d], grad_b_ih, grad_b_hh [3d]; with ``Ws_next``
    [a, d], ``g_as`` [n, >= a] and the saved ``hidden`` also grad_Ws [a, d], and everything else from the effective
    grad_hidden = grad_hidden + g_as[:, :a] Ws_next (models._DenseStep.backward)."""
    from tests import gram_ref      # imports this module: not at the top
    act = ACT.get(act, act)
    keep = float(np.float32(keep))      # the kernels take keep as a C float
    dt = np.dtype(dtype)
    g, S_g, extra = _c(dt, grad_hidden), np.abs(np.asarray(grad_hidden, np.float64)), 0
    if Ws_next is not None:
        a = np.shape(Ws_next)[0]
        g = g + _c(dt, g_as)[:, :a] @ _c(dt, Ws_next)
        S_g = S_g + np.abs(np.asarray(g_as, np.float64)[:, :a]) @ np.abs(np.asarray(Ws_next, np.float64))
        extra = a + 1
    args = (ws, x, mask, keep, act, W_h, w_ih, w_hh)
    v = _bwd_values(dt, g, *args, absolute=False, fault=fault)
    S = _bwd_values(np.dtype(np.float64), S_g, *args, absolute=True)
    d = np.shape(x)[1]
    n = dict(dgi=0, dgh=0, dgh_n=0, dpre=3 * d, dagg=4 * d, dh0=3 * d + 1, grad_prev=3 * d + 1)
    n = {k: t + extra for k, t in n.items()}
    v["grad_prev"], S["grad_prev"] = _scatter_prev(v["dh0"], prev_idx, n_old), _scatter_prev(S["dh0"], prev_idx, n_old)
    v["grad_hidden"], S["grad_hidden"], n["grad_hidden"] = g, S_g, extra
    if agg is not None:
        rows = np.shape(x)[0]
        h0 = np.asarray(ws).reshape(rows, 5, d)[:, 3]
        n_out, n_cs = gram_ref.n_terms(rows)
        absolute = lambda t: np.abs(np.asarray(t, np.float64))
        prods = [("grad_W_h", "dpre", agg, None), ("grad_w_ih", "dgi", x, "grad_b_ih"), ("grad_w_hh", "dgh", h0, "grad_b_hh")]
        for name, left, right, bias in prods:
            r = gram_ref.gram(v[left], _c(dt, right), dt)
            v[name], S[name], n[name] = r.out, S[left].T @ absolute(right), n[left] + n_out
            if bias:
                v[bias], S[bias], n[bias] = r.colsum, S[left].sum(0), n[left] + n_cs
        if Ws_next is not None:
            v["grad_Ws"] = gram_ref.gram(_c(dt, g_as)[:, :a], _c(dt, hidden), dt).out
            S["grad_Ws"], n["grad_Ws"] = absolute(g_as)[:, :a].T @ absolute(hidden), n_out
        if fault == "cat_order":
            v["grad_w_hh"], v["grad_b_hh"] = _cat_order(v["grad_w_hh"], d), _cat_order(v["grad_b_hh"], d)
    return types.SimpleNamespace(S=S, n=n, **v)


# ---- the two row-wise products --------------------------------------------------------------------------------------------------------
def rows_addmm(base, g, W, dtype=np.float64):
    """out = base + g[:, :k] W for W [k, n] (include/redgnn.h, rg_rows_addmm); the sum runs j = 0 .. k - 1 onto base, as a row's thread
    does."""
    dt = np.dtype(dtype)
    k = np.shape(W)[0]
    b, gg, w = _c(dt, base), _c(dt, g)[:, :k], _c(dt, W)
    out = b.copy()
    for j in range(k):
        out = out + gg[:, j:j + 1] * w[j:j + 1]
    S = np.abs(np.asarray(base, np.float64)) + np.abs(np.asarray(g, np.float64)[:, :k]) @ np.abs(np.asarray(W, np.float64))
    return types.SimpleNamespace(out=out, S=dict(out=S), n=dict(out=k + 1))


def attn_tables(rela, Wr, Wqr, bqr, q_rel, ap, ld, dtype=np.float64):
    """One layer of rg_attn_tables: a_r [rows, ap], a_q [B, ap] (columns attn_dim .. ap - 1 zero), rela_pad [rows, ld] (the table with
    zero columns d .. ld - 1; a bit copy)."""
    dt = np.dtype(dtype)
    r, wr, wq, b = _c(dt, rela), _c(dt, Wr), _c(dt, Wqr), _c(dt, bqr)
    rows, d = r.shape
    attn = wr.shape[0]
    q = np.asarray(q_rel, np.int64)
    a_r, a_q = np.zeros((rows, ap), dt), np.zeros((len(q), ap), dt)
    a_r[:, :attn] = r @ wr.T
    a_q[:, :attn] = r[q] @ wq.T + b
    pad = np.zeros((rows, ld), dt)
    pad[:, :d] = r
    A = lambda t: np.abs(np.asarray(t, np.float64))
    S_r, S_q = np.zeros((rows, ap)), np.zeros((len(q), ap))
    S_r[:, :attn] = A(rela) @ A(Wr).T
    S_q[:, :attn] = A(rela)[q] @ A(Wqr).T + A(bqr)
    return types.SimpleNamespace(a_r=a_r, a_q=a_q, rela_pad=pad, S=dict(a_r=S_r, a_q=S_q), n=dict(a_r=d, a_q=d + 1))


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# One entry per dispatch condition; ``why`` cites the line the case flips.  A step case runs the training forward (rg_dense_train_fwd,
# or _fwd_as when attn_dim > 0) and, for d <= 64, both backward entries on the saved outputs of the fp64 forward, rounded once.
# These are direct calls: every kernel gets every row count, not only the ones models._DenseStep would route to it.
def _step(name, d, n, act="relu", masked=False, prev="third", attn_dim=0, seed=0, why=""):
    return types.SimpleNamespace(name=name, kind="step", d=d, n=n, act=ACT[act], masked=masked, keep=0.7, prev=prev, attn_dim=attn_dim,
                                 ap=(attn_dim + 3) // 4 * 4, seed=seed, why=why, fwd_only=d == 128)


def _addmm(name, cols, k, n_rows, g_width=None, base_width=None, alias=False, seed=0, why=""):
    return types.SimpleNamespace(name=name, kind="addmm", cols=cols, k=k, n_rows=n_rows, g_width=k if g_width is None else g_width,
                                 base_width=cols if base_width is None else base_width, alias=alias, seed=seed, why=why)


def _tables(name, n_layer, d, ld, attn_dim, ap, n_rows=11, B=9, seed=0, why=""):
    return types.SimpleNamespace(name=name, kind="tables", n_layer=n_layer, d=d, ld=ld, attn_dim=attn_dim, ap=ap, n_rows=n_rows, B=B,
                                 seed=seed, why=why)


_CASE_LIST = [
    # ---- width: dense.hip launch<2> / dense_bwd.hip launch_bwd<2> for d <= 32, <4> above; `col < d` leaves the last 16-column block
    # partly empty at d = 20, 36, 60 (dense_bwd.hip fetch / stores, dense.hip TRAIN stores)
    _step("d16_relu", 16, 1000, "relu", False, "third", seed=1, why="dense_bwd.hip:240 d <= 32 -> NB = 2, full blocks"),
    _step("d20_tanh_mask", 20, 1000, "tanh", True, "all", seed=2, why="NB = 2, block 1 holds 4 of 16 columns (col < d)"),
    _step("d32_idd", 32, 1000, "idd", False, "none", seed=3, why="NB = 2 at its upper edge"),
    _step("d36_relu_mask", 36, 1000, "relu", True, "third", seed=4, why="dense_bwd.hip:240 d > 32 -> NB = 4, block 2 holds 4 columns, block 3 none"),
    _step("d48_tanh", 48, 1000, "tanh", False, "null", seed=5, why="NB = 4, block 3 empty"),
    _step("d60_idd_mask", 60, 1000, "idd", True, "third", seed=6, why="NB = 4, block 3 holds 12 columns"),
    _step("d64_relu_mask", 64, 1000, "relu", True, "all", seed=7, why="NB = 4, full blocks"),
    _step("d64_tanh_mask", 64, 1000, "tanh", True, "third", seed=8, why="dense_bwd.hip:179 y = x * keep under a mask"),
    _step("d128_relu", 128, 300, "relu", False, "third", seed=9, why="dense.hip:418 d == 128 -> dense128_launch (forward only)"),
    _step("d128_tanh_mask", 128, 2049, "tanh", True, "all", seed=10, why="dense128.hip TRAIN with a mask"),
    # ---- rows around the 16-row tile (n_tiles = ceil(n / 16); in_n guards)
    _step("n1", 64, 1, "relu", True, "all", seed=11, why="one row of one tile"),
    _step("n15", 32, 15, "tanh", False, "third", seed=12, why="tile short of one row"),
    _step("n16", 64, 16, "idd", True, "third", seed=13, why="exactly one tile"),
    _step("n17", 36, 17, "relu", False, "all", seed=14, why="one row into the second tile"),
    # ---- rows around models.py _FUSED_BWD_ROWS = 8192 and _TALL_ROWS = 32768 (what _DenseStep routes by)
    _step("n8191", 48, 8191, "relu", True, "third", seed=15, why="models.py:176 below _FUSED_BWD_ROWS"),
    _step("n8193", 16, 8193, "tanh", True, "all", seed=16, why="models.py:176 above _FUSED_BWD_ROWS"),
    _step("n32767", 64, 32767, "tanh", False, "third", seed=17, why="models.py:166 below _TALL_ROWS; one full pass of the persistent grid less a row"),
    _step("n32769", 64, 32769, "relu", True, "third", attn_dim=5, seed=18, why="models.py:166 above _TALL_ROWS; the grid-stride loop's second pass: one row"),
    # ---- the persistent grid's second pass full and a third begun: 256 workgroups x 8 waves x 16 rows = 32768 rows per pass
    _step("n70001_d64", 64, 70001, "relu", True, "third", seed=19, why="dense_bwd.hip:89 / dense.hip:183 t += gridDim.x * NW, two full passes"),
    _step("n70001_d20", 20, 70001, "idd", False, "all", attn_dim=8, seed=20, why="the same with NB = 2 and a partly filled block"),
    _step("n70001_d128", 128, 70001, "idd", False, "none", seed=21, why="dense128.hip persistent grid"),
    # ---- rg_dense_train_fwd_as: attn_dim 1, 5, 8, 16 (ap 4, 8, 8, 16; `4 * hq < A.ap` store guard, pad columns zero)
    _step("as1", 64, 1000, "relu", False, "third", attn_dim=1, seed=22, why="dense.hip:289 ap = 4: one lane quarter stores"),
    _step("as5", 48, 1000, "tanh", True, "third", attn_dim=5, seed=23, why="ap = 8, three pad columns"),
    _step("as8", 32, 1000, "idd", False, "all", attn_dim=8, seed=24, why="ap = 8, no pad"),
    _step("as16", 20, 1000, "relu", True, "null", attn_dim=16, seed=25, why="ap = 16: all four lane quarters store"),
    _step("as16_d128", 128, 1000, "tanh", False, "third", attn_dim=16, seed=26, why="dense128.hip:276 a_s store"),
    # ---- rg_rows_addmm: columns 16 .. 128 (per_block = 256 / (n / 4): 64, 32, 21 with 4 idle threads, 16, 8), k 1, 5, 16, 32
    _addmm("am16_k1", 16, 1, 1000, seed=30, why="gram.hip:198 per_block = 64"),
    _addmm("am32_k5", 32, 5, 1000, g_width=8, seed=31, why="per_block = 32; g = a column block of a wider buffer (ldg > k)"),
    _addmm("am48_k16", 48, 16, 70001, seed=32, why="gram.hip:200 per_block = 21: threads 252 .. 255 idle; 2048 workgroups' grid-stride loop"),
    _addmm("am64_k32", 64, 32, 33000, g_width=40, base_width=192, seed=33, why="k at its limit; spaced base rows (ldb = 192) and ldg = 40"),
    _addmm("am128_k5", 128, 5, 1000, g_width=8, alias=True, seed=34, why="n at its limit (per_block = 8); out aliases base"),
    _addmm("am48_k5_alias", 48, 5, 17, g_width=8, alias=True, seed=35, why="fewer rows than one workgroup pass; out aliases base"),
    # ---- rg_attn_tables (rank.hip attn_tables_kernel): layers, ld != d copy, pad columns, repeated query relations, 475 rows
    _tables("t1_ld_eq", 1, 64, 64, 5, 8, seed=40, why="rank.hip:143 ld == d: no rela_pad"),
    _tables("t3_d30_ld32", 3, 30, 32, 3, 4, seed=41, why="rank.hip:121 the ld != d copy, d % 4 != 0"),
    _tables("t5_d48_ld64", 5, 48, 64, 16, 32, seed=42, why="five layers; attn_dim 16 in ap 32: half the columns are pad"),
    _tables("t3_475rows", 3, 128, 128, 5, 8, n_rows=475, B=64, seed=43, why="475 relation rows (n_rel = 237), a batch of repeated relations"),
]
CASES = {c.name: c for c in _CASE_LIST}


def _prev(rng, mode, n):
    """(prev_idx int32 [n] or None, n_old): NULL; all -1; a third of the rows old; every row old (a permutation)."""
    if mode == "null":
        return None, 0
    if mode == "none":
        return np.full(n, -1, np.int32), 0
    n_old = n if mode == "all" else (n + 2) // 3
    p = np.full(n, -1, np.int32)
    p[rng.choice(n, n_old, replace=False)] = rng.permutation(n_old).astype(np.int32)
    return p, n_old


def inputs(case):
    """Seeded random inputs of a case: dict of float32 arrays (prev_idx int32, q_rel int64) in the kernels' layouts."""
    rng = np.random.default_rng(500 + case.seed)
    f = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(np.float32)
    if case.kind in ("step", "route"):
        d, n = case.d, case.n
        prev_idx, n_old = _prev(rng, case.prev, n)
        x = dict(agg=f(n, d), prev_idx=prev_idx, n_old=n_old,
                 hidden_prev=None if prev_idx is None else np.clip(f(max(n_old, 1), d, scale=0.5), -1, 1),
                 W_h=f(d, d, scale=d ** -0.5), w_ih=f(3 * d, d, scale=d ** -0.5), w_hh=f(3 * d, d, scale=d ** -0.5),
                 b_ih=f(3 * d, scale=0.3), b_hh=f(3 * d, scale=0.3),
                 mask=((rng.random((n, d)) < case.keep) / np.float32(case.keep)).astype(np.float32) if case.masked else None,
                 Ws_next=f(case.attn_dim, d, scale=d ** -0.5) if case.attn_dim else None, grad_hidden=f(n, d))
        if case.kind == "route" and case.attn_dim:
            x["g_as"] = f(n, case.ap)      # the pad columns attn_dim .. ap - 1 carry values too: nothing may read them
        return x
    if case.kind == "addmm":
        return dict(base=f(case.n_rows, case.base_width), g=f(case.n_rows, case.g_width), W=f(case.k, case.cols, scale=case.k ** -0.5))
    q_rel = rng.integers(0, case.n_rows, case.B).astype(np.int64)
    q_rel[1::2] = q_rel[0]      # every other query repeats the first one's relation
    q_rel[-1] = case.n_rows - 1
    return dict(q_rel=q_rel, rela=[f(case.n_rows, case.d) for _ in range(case.n_layer)],
                Wr=[f(case.attn_dim, case.d, scale=case.d ** -0.5) for _ in range(case.n_layer)],
                Wqr=[f(case.attn_dim, case.d, scale=case.d ** -0.5) for _ in range(case.n_layer)],
                bqr=[f(case.attn_dim, scale=0.3) for _ in range(case.n_layer)])


def step_forward(case, x, dtype=np.float64, fault=None):
    return forward(x["agg"], x["hidden_prev"], x["prev_idx"], x["W_h"], case.act, x["w_ih"], x["w_hh"], x["b_ih"], x["b_hh"], x["mask"],
                   x["Ws_next"], case.ap if case.attn_dim else None, dtype=dtype, fault=fault)


def saved(case, x):
    """What the backward kernels are fed: x and ws of the fp64 forward, rounded once to fp32 (ws as [n, 5 d])."""
    f = step_forward(case, x)
    return f.x.astype(np.float32), f.ws.astype(np.float32).reshape(case.n, 5 * case.d)


def step_backward(case, x, x_saved, ws_saved, dtype=np.float64, fault=None):
    return backward(x["grad_hidden"], ws_saved, x_saved, x["mask"], case.keep, case.act, x["W_h"], x["w_ih"], x["w_hh"], x["prev_idx"],
                    x["n_old"], dtype=dtype, fault=fault)


# ---- the routes of models._DenseStep.backward -------------------------------------------------------------------------------------------
# One entry per route and width; ``why`` cites the line of red-gnn_amd/models.py the case selects.  A route case runs
# models._DenseStep.apply forward and backward and checks every gradient it returns against ``backward`` (with agg) on the x / ws the
# step saved.  Rows: no more than the routing thresholds need (_FUSED_BWD_ROWS = 8192, _TALL_ROWS = 32768).
def _route(name, d, n, act="relu", masked=False, prev="third", attn_dim=0, seed=0, why=""):
    c = _step(name, d, n, act, masked, prev, attn_dim, seed, why)
    c.kind = "route"
    return c


_ROT = [("relu", True), ("tanh", False), ("idd", True), ("relu", False), ("tanh", True), ("idd", False)]      # act, mask over the widths
_BWD2 = "models.py:166 n >= _TALL_ROWS with old rows -> rg_dense_train_bwd2; models.py:172-174 engine.gram_tn: "
_ROUTE_LIST = (
    [_route("bwd2_d%d" % d, d, 32768, *_ROT[i % 6], prev="third", seed=60 + i,
            why=_BWD2 + "dgi^T x (m = %d), dgi[:, :2d]^T h0 (m = %d, h0 the ws.view(n, 5, d)[:, 3] view), dgh_n^T h0, dpre^T agg (m = n = %d); "
            "models.py:175 torch.cat([g_rz, g_n]) / ([db_rz, db_n])" % (3 * d, 2 * d, d)) for i, d in enumerate(range(16, 65, 4))]
    + [_route("bwd2_d%d_as%d" % (d, a), d, 32768, *_ROT[(i + a) % 6], prev="third", attn_dim=a, seed=80 + 2 * i + (a == 16),
              why=_BWD2 + "with Ws_next: models.py:164 _gram_tn(g_as[:, :a], hidden) -> models.py:68 engine.gram_tn (m = %d, ldg = %d) and "
              "models.py:165 engine.rows_addmm" % (a, (a + 3) // 4 * 4)) for i, d in enumerate((20, 48, 64)) for a in (5, 16)]
    + [_route("bwd_d%d" % d, d, 32768, *_ROT[(i + 2) % 6], prev="none", seed=90 + i,
              why="models.py:166 n_old = 0 -> not bwd2; models.py:176 rg_dense_train_bwd; models.py:180-182 n >= _TALL_ROWS: engine.gram_tn(dgi, x), "
              "(dgh, h0) with colsum, (dpre, agg)") for i, d in enumerate((16, 36, 64))]
    + [_route("sums_n8192", 32, 8192, "tanh", True, "third", seed=95,
              why="models.py:176 n >= _FUSED_BWD_ROWS -> rg_dense_train_bwd; models.py:185 dgi.sum(0) / dgh.sum(0); models.py:201-202 _gram_tn -> "
              "models.py:66 g.t() @ x below _TALL_ROWS"),
       _route("sums_n32767", 32, 32767, "relu", True, "third", seed=96, why="the same one row below models.py:180 _TALL_ROWS"),
       _route("aten_n8191", 32, 8191, "tanh", True, "third", seed=97,
              why="models.py:176 one row below _FUSED_BWD_ROWS -> models.py:187 aten's GRU-cell backward, three GEMMs; models.py:201-202"),
       _route("aten_d128", 128, 32768, "relu", True, "third", seed=98,
              why="models.py:176 dense_train_bwd_supported(128) false -> models.py:187 aten; models.py:201-202 _gram_tn -> models.py:68 engine.gram_tn "
              "tiled 384 x 128 (engine.py:743)")]
)
ROUTE_CASES = {c.name: c for c in _ROUTE_LIST}


def route_backward(case, x, x_saved, ws_saved, hidden_saved=None, dtype=np.float64, fault=None):
    """``backward`` with the weight gradients on what a route case's step saved."""
    extra = dict(g_as=x["g_as"], Ws_next=x["Ws_next"], hidden=hidden_saved) if case.attn_dim else {}
    return backward(x["grad_hidden"], ws_saved, x_saved, x["mask"], case.keep, case.act, x["W_h"], x["w_ih"], x["w_hh"], x["prev_idx"],
                    x["n_old"], dtype=dtype, fault=fault, agg=x["agg"], **extra)


# ---- the inference contract (rg_dense_fwd / rg_dense_fwd_dev, precisions 0, 1, 2) ------------------------------------------------------
# Outputs: hidden [n, d], a_s [n, ap] (with Ws_next), score [n] scattered by nodes (with W_final).  Precisions 0 (f32 MFMA) and 2 (exact
# three-term f16 split: "fp32 arithmetic", include/redgnn.h) are held to ``bound`` with C_BOUND, like the training kernels.  Precision 1
# carries every operand of a matrix product to 22 bits and gets one added term
#
#     |gpu - ref64| <= C_BOUND (n + n0) u S  +  C2_F16X2 p 2^-22 S  +  tiny
#
# with p = the number of matrix products chained into the element (P_CHAIN).  C2_F16X2 is 2 x the worst ratio
# |emul - ref64| / (p 2^-22 S) of ``forward_f16x2`` below - the two-term operand form of csrc/split3.h in numpy, everything else in fp64 -
# over the inference table.  2 rather than 4: the operand roundings are deterministic and the same in the kernel and in the emulation;
# only their inputs differ, by the fp32 error the first term pays for.
INFER_OUTPUTS = ("hidden", "a_s", "score")
P_CHAIN = dict(x=1, hidden=2, a_s=3, score=3)
U22 = 2.0 ** -22
# measured: max over the inference table, outputs and elements of |forward_f16x2 - ref64| / (p 2^-22 S), rounded up
# (test_dense_ref.py::test_f16x2_emulation_ratio_is_the_recorded_one keeps it honest)
REF_F16X2_WORST_RATIO = 0.125      # spike_d20_ld32's hidden: 0.124
C2_F16X2 = 2.0 * REF_F16X2_WORST_RATIO


def bound_f16x2(S, n, n0, p):
    return bound(S, n, n0, C_BOUND) + C2_F16X2 * p * U22 * np.asarray(S, np.float64)


def infer_bound(precision, S, n, out):
    """The allowance of output ``out`` at ``precision`` (0 f32, 1 f16x2, 2 f16x3)."""
    return bound_f16x2(S, n, N0_STEP, P_CHAIN[out]) if precision == 1 else bound(S, n, N0_STEP, C_BOUND)


def _pow2_scale(m, top):
    """The power of two that takes m (>= 0) into [2^(top - 1), 2^top); 1 for m = 0."""
    m = np.asarray(m, np.float64)
    _, e = np.frexp(m)      # m = f 2^e, f in [1/2, 1)
    return np.where(m > 0, np.ldexp(1.0, top - e), 1.0)


def _split2(v, s):
    """hi = f16(v s), lo = f16(v s - hi) (numpy's float16: round to nearest even, subnormals kept), as fp64."""
    vs = np.asarray(v, np.float64) * s
    hi = vs.astype(np.float16).astype(np.float64)
    lo = (vs - hi).astype(np.float16).astype(np.float64)
    return hi, lo


def _prod2(X, sx, W, sw, fault=None):
    """X W^T with both operands as two-term splits: (W_hi X_hi + W_hi X_lo + W_lo X_hi) / (sx sw), the sums in fp64.
    fault "no_lo_hi": the W_lo X_hi term dropped; "one_term": hi halves only (negative tests only)."""
    xh, xl = _split2(X, sx)
    wh, wl = _split2(W, sw)
    acc = xh @ wh.T
    if fault != "one_term":
        acc = acc + xl @ wh.T
        if fault != "no_lo_hi":
            acc = acc + xh @ wl.T
    return acc / (sx * sw)


def forward_f16x2(agg, hidden_prev, prev_idx, W_h, act, w_ih, w_hh, b_ih, b_hh, Ws_next=None, ap=None, W_final=None, fault=None):
    """The step with the operands of every matrix product in the two-term f16 form csrc/split3.h documents - a power-of-two scale per
    node row that takes the row's largest magnitude into [2^14, 2^15) (x and h0 of a row share one, so that W_ih x and W_hh h0 add in
    one accumulator), one per launch that takes the largest weight of the layer's seven matrices into [2^13, 2^14) and one of their own
    for the projections (split3.h:149-158, dense_split.hip, dense_split3.hip:82), hi = f16(v s), lo = f16(v s - hi), products hi hi + hi lo + lo hi - and everything
    else (sums, biases, sigmoid, tanh, the state update) in fp64.  hidden, x, a_s, score as ``forward``."""
    act = ACT.get(act, act)
    f = lambda t: None if t is None else np.asarray(t, np.float64)
    agg, hidden_prev, W_h, w_ih, w_hh, b_ih, b_hh, Ws_next, W_final = (f(t) for t in (agg, hidden_prev, W_h, w_ih, w_hh, b_ih, b_hh, Ws_next,
                                                                                    W_final))
    n, d = agg.shape
    amax = lambda *ts: max([float(np.abs(t).max()) for t in ts if t is not None and t.size] + [0.0])
    sw_g, sw_e = float(_pow2_scale(amax(W_h, w_ih, w_hh), 14)), float(_pow2_scale(amax(Ws_next, W_final), 14))
    rows = lambda *ts: _pow2_scale(np.max([np.abs(t).max(1) for t in ts], 0), 15)[:, None]
    h0 = _gather(hidden_prev, prev_idx, n, d, np.dtype(np.float64))
    pre = _prod2(agg, rows(agg), W_h, sw_g, fault)
    x = pre if act == 0 else np.maximum(pre, 0.0) if act == 1 else np.tanh(pre)
    s = rows(x, h0)
    gi = _prod2(x, s, w_ih, sw_g, fault) + b_ih
    hh = _prod2(h0, s, w_hh, sw_g, fault)
    r = _sigmoid(gi[:, :d] + hh[:, :d] + b_hh[:d])
    z = _sigmoid(gi[:, d:2 * d] + hh[:, d:2 * d] + b_hh[d:2 * d])
    ng = np.tanh(gi[:, 2 * d:] + r * (hh[:, 2 * d:] + b_hh[2 * d:]))
    hidden = (1.0 - z) * ng + z * h0
    sh = rows(hidden)
    a_s = None
    if Ws_next is not None:
        attn = Ws_next.shape[0]
        a_s = np.zeros((n, (attn + 3) // 4 * 4 if ap is None else ap))
        a_s[:, :attn] = _prod2(hidden, sh, Ws_next, sw_e, fault)
    score = None if W_final is None else _prod2(hidden, sh, W_final[None], sw_e, fault)[:, 0]
    return types.SimpleNamespace(hidden=hidden, x=x, a_s=a_s, score=score)


# The inference table: one entry per dispatch condition of the six fused kernels (csrc/dense.hip, dense_split.hip, dense_split3.hip for
# d <= 64; dense128.hip, dense128_split.hip, dense128_split3.hip for d = 128); ``why`` cites the line the case flips.  Every case runs at
# the precisions in ``precisions`` (all three unless the case says otherwise).  agg / hidden_prev come with their true d columns: padding
# the rows to ld (zero pad columns) is the test's business.
def _infer(name, d, n, ld=None, act="relu", prev="third", attn_dim=0, readout=False, no_hidden=False, rows="plain", ws_scale=1.0,
           precisions=(0, 1, 2), seed=0, why=""):
    return types.SimpleNamespace(name=name, kind="infer", d=d, ld=d if ld is None else ld, n=n, act=ACT[act], prev=prev, attn_dim=attn_dim,
                                 ap=(attn_dim + 3) // 4 * 4, readout=readout, no_hidden=no_hidden, rows=rows, ws_scale=ws_scale,
                                 precisions=precisions, seed=seed, why=why)


# rows per pass of the persistent grid: 256 workgroups x NW waves x 16 rows (dense_common.h:67 dense_grid).  NW = 8 in dense.hip:42,
# dense_split.hip:32, dense_split3.hip:35, dense128.hip:19, dense128_split.hip:19; NW = 4 in dense128_split3.hip:25
ROWS_PER_PASS = {8: 256 * 8 * 16, 4: 256 * 4 * 16}

_INFER_LIST = [
    # ---- width and stride: DP = 32 for d <= 32, 64 above (dense.hip:366, dense_split.hip:342, dense_split3.hip launch_act); the weight
    # staging's `c < d` guards (dense.hip:69, dense_split.hip:69, dense_split3.hip:100) on rows of stride ld4, the state store's `sl < ld4`
    _infer("w_d1_ld4", 1, 1000, 4, "tanh", "runs", 1, True, seed=1, why="dense.hip:69 scalar staging, one column; one float4 per row (ld4 = 1)"),
    _infer("w_d3_ld4", 3, 1000, 4, "relu", "third", 5, True, seed=2, why="d % 4 != 0 and d < 16: one pad column inside the only float4"),
    _infer("w_d20", 20, 1000, 20, "idd", "runs", 5, True, seed=3, why="ld4 = 5: block 1 holds one float4 of four (col_ok, dense_split.hip:165)"),
    _infer("w_d20_ld32", 20, 1000, 32, "relu", "all", 8, True, seed=4, why="ld > d with d % 4 == 0: vector staging, three pad float4 stored"),
    _infer("w_d30_ld32", 30, 1000, 32, "tanh", "runs", 5, True, seed=5, why="dense_split3.hip:100 scalar staging, two pad columns in the last float4"),
    _infer("w_d32", 32, 1000, 32, "idd", "third", 16, True, seed=6, why="DP = 32 at its upper edge"),
    _infer("w_d33_ld36", 33, 1000, 36, "relu", "runs", 5, True, seed=7, why="d > 32 -> DP = 64 by one column; scalar staging; ld4 = 9"),
    _infer("w_d48_ld64", 48, 1000, 64, "tanh", "third", 8, True, seed=8, why="DP = 64, block 3 all pad and stored"),
    _infer("w_d63_ld64", 63, 1000, 64, "idd", "runs", 5, True, seed=9, why="scalar staging at DP = 64, one pad column"),
    _infer("w_d64", 64, 1000, 64, "relu", "runs", 5, True, seed=10, why="DP = 64, full blocks"),
    _infer("w_d128", 128, 1000, 128, "tanh", "runs", 5, True, seed=11, why="dense.hip:361 d == 128 -> the streamed-weight kernels"),
    # ---- rows around the 16-row tile (n_tiles = ceil(n / 16); node_ok / rows_valid guards, dense_split3.hip:307)
    _infer("n1_d64", 64, 1, act="relu", prev="all", attn_dim=5, readout=True, seed=12, why="one row of one tile"),
    _infer("n15_d64", 64, 15, act="tanh", prev="third", attn_dim=8, readout=True, seed=13, why="tile short of one row"),
    _infer("n16_d64", 64, 16, act="idd", prev="third", attn_dim=5, readout=True, seed=14, why="exactly one tile"),
    _infer("n17_d64", 64, 17, act="relu", prev="all", attn_dim=16, readout=True, seed=15, why="one row into the second tile"),
    _infer("n1_d128", 128, 1, act="tanh", prev="all", attn_dim=5, readout=True, seed=16, why="d = 128: one row of one tile"),
    _infer("n15_d128", 128, 15, act="relu", prev="third", attn_dim=8, readout=True, seed=17, why="d = 128: tile short of one row"),
    _infer("n16_d128", 128, 16, act="idd", prev="third", attn_dim=5, readout=True, seed=18, why="d = 128: exactly one tile"),
    _infer("n17_d128", 128, 17, act="relu", prev="all", attn_dim=16, readout=True, seed=19, why="d = 128: one row into the second tile"),
    # ---- the persistent grid's second pass (t += gridDim.x * NW: dense.hip:184, dense_split.hip:195, dense_split3.hip:243)
    _infer("n32769_d64", 64, ROWS_PER_PASS[8] + 1, act="relu", prev="runs", attn_dim=5, readout=True, seed=20,
           why="NW = 8: 32768 rows per pass, the second pass one row"),
    _infer("n32769_d20", 20, ROWS_PER_PASS[8] + 1, act="tanh", prev="third", attn_dim=8, readout=True, seed=21,
           why="the same at DP = 32 with a partly filled block"),
    _infer("n32769_d128", 128, ROWS_PER_PASS[8] + 1, act="idd", prev="runs", attn_dim=5, readout=True, precisions=(0, 1), seed=22,
           why="dense128.hip:19 / dense128_split.hip:19 NW = 8"),
    _infer("n16385_d128", 128, ROWS_PER_PASS[4] + 1, act="relu", prev="runs", attn_dim=5, readout=True, precisions=(2,), seed=23,
           why="dense128_split3.hip:25 NW = 4: 16384 rows per pass"),
    # ---- prev_idx: NULL, all -1, every row old, a third at random, and runs of 1 .. 40 old / new rows (whole tiles all new, all old and
    # mixed next to one another: any_old, dense.hip:263, dense_split.hip:307, dense_split3.hip:251/544)
    _infer("prev_null", 48, 1000, act="relu", prev="null", attn_dim=5, seed=24, why="prev_idx NULL: no gather at all"),
    _infer("prev_none", 64, 1000, act="tanh", prev="none", attn_dim=5, seed=25, why="prev_idx given, every entry -1: any_old false in every tile"),
    _infer("prev_all", 32, 1000, act="idd", prev="all", attn_dim=5, seed=26, why="any_old true in every tile, no new row"),
    _infer("prev_third", 64, 1000, act="relu", prev="third", attn_dim=5, seed=27, why="every tile mixed"),
    _infer("prev_runs_d64", 64, 2000, act="tanh", prev="runs", attn_dim=5, seed=28, why="any_old true and false inside one call, DP = 64"),
    _infer("prev_runs_d20", 20, 2000, act="relu", prev="runs", attn_dim=5, seed=29, why="any_old true and false inside one call, DP = 32"),
    _infer("prev_runs_d128", 128, 2000, act="idd", prev="runs", attn_dim=5, seed=30, why="d = 128: old and new tiles in one call"),
    # ---- projection and readout: attn_dim 1, 5, 8, 16 (ap 4, 8, 8, 16: `4 * hq < A.ap`), W_final scattered by sorted distinct
    # (query, entity) pairs with gaps, neither, hidden_out = NULL on a readout
    _infer("as1", 64, 1000, act="relu", prev="third", attn_dim=1, seed=31, why="dense.hip:290 ap = 4: one lane quarter stores"),
    _infer("as5", 48, 1000, act="tanh", prev="runs", attn_dim=5, seed=32, why="ap = 8, three pad columns"),
    _infer("as8", 32, 1000, act="idd", prev="all", attn_dim=8, seed=33, why="ap = 8, no pad"),
    _infer("as16", 20, 1000, act="relu", prev="third", attn_dim=16, seed=34, why="ap = 16: all four lane quarters store"),
    _infer("as16_d128", 128, 1000, act="tanh", prev="third", attn_dim=16, seed=35, why="d = 128 a_s store, block 56 of the image"),
    _infer("readout", 64, 1000, act="relu", prev="runs", readout=True, seed=36, why="dense.hip:293 W_final only: row 16 of E, scatter by nodes"),
    _infer("readout_d128", 128, 1000, act="idd", prev="third", readout=True, seed=37, why="d = 128: block 57 of the image"),
    _infer("neither", 48, 1000, act="tanh", prev="third", seed=38, why="neither Ws_next nor W_final: the state alone"),
    _infer("neither_d128", 128, 1000, act="relu", prev="runs", seed=39, why="d = 128: the state alone"),
    _infer("no_hidden", 64, 1000, act="tanh", prev="runs", readout=True, no_hidden=True, seed=40,
           why="dense.hip:312 / dense_split.hip:295 / dense_split3.hip:310 hidden_out = NULL: no state store"),
    _infer("no_hidden_d20_ld32", 20, 1000, 32, act="relu", prev="third", readout=True, no_hidden=True, seed=41, why="the same at DP = 32, ld > d"),
    _infer("no_hidden_d128", 128, 1000, act="idd", prev="runs", readout=True, no_hidden=True, seed=42, why="d = 128 without the state store"),
    # ---- row scales of the split kernels: row_scale(row_abs_max(..)) per node row (dense_common.h:111, split3.h:121), shared by x and h0 in
    # the GRU (dense_split.hip:258, dense_split3.hip:321)
    _infer("spike_d64", 64, 1000, act="idd", prev="runs", attn_dim=5, readout=True, rows="spike", seed=43,
           why="the row's largest element in every column in turn, 8 x the rest: a maximum the quarter-wave shuffles miss overflows f16"),
    _infer("spike_d20_ld32", 20, 1000, 32, act="relu", prev="third", attn_dim=5, readout=True, rows="spike", seed=44, why="the same at DP = 32, ld > d"),
    _infer("spike_d128", 128, 1000, act="idd", prev="runs", attn_dim=5, readout=True, rows="spike", seed=45, why="the same at d = 128"),
    _infer("x_over_h_d64", 64, 1000, act="idd", prev="runs", attn_dim=5, readout=True, rows="x_over_h", seed=46,
           why="agg x 100: |x| >> |h0| under the shared GRU scale"),
    _infer("x_over_h_d128", 128, 1000, act="idd", prev="third", attn_dim=5, readout=True, rows="x_over_h", seed=47, why="the same at d = 128"),
    _infer("h_over_x_d64", 64, 1000, act="idd", prev="runs", attn_dim=5, readout=True, rows="h_over_x", seed=48,
           why="agg x 1e-3: |h0| >> |x| under the shared GRU scale"),
    _infer("h_over_x_d128", 128, 1000, act="idd", prev="third", attn_dim=5, readout=True, rows="h_over_x", seed=49, why="the same at d = 128"),
    # ---- weight scale: Ws_next x 300 with the gate weights at unit scale
    _infer("ws300_d64", 64, 1000, act="relu", prev="runs", attn_dim=5, ws_scale=300.0, seed=50,
           why="dense_split.hip the projections' scale refitted, the layer's kept; dense_split3.hip:82 the projections' own"),
    _infer("ws300_d128", 128, 1000, act="tanh", prev="third", attn_dim=5, ws_scale=300.0, seed=51, why="split3.h:149-158 the projections' own scale"),
]
INFER_CASES = {c.name: c for c in _INFER_LIST}


def _prev_runs(rng, n):
    """Old and new rows in alternating runs of 1 .. 40 rows (seeded lengths): (prev_idx, n_old)."""
    old = np.zeros(n, bool)
    at, state = 0, bool(rng.integers(0, 2))
    while at < n:
        length = int(rng.integers(1, 41))
        old[at:at + length] = state
        at, state = at + length, not state
    n_old = int(old.sum())
    p = np.full(n, -1, np.int32)
    p[old] = rng.permutation(n_old).astype(np.int32)
    return p, n_old


def tile_census(prev_idx, n):
    """(all new, all old, mixed): how many 16-row tiles of the call have no old row, only old rows, both."""
    old = np.zeros(n, bool) if prev_idx is None else np.asarray(prev_idx) >= 0
    kinds = [(bool(old[t:t + 16].any()), bool(old[t:t + 16].all())) for t in range(0, n, 16)]
    return sum(not a for a, _ in kinds), sum(b for _, b in kinds), sum(a and not b for a, b in kinds)


def infer_inputs(case):
    """Seeded inputs of an inference case: float32 arrays with the true d columns (prev_idx int32 [n] or None, nodes int32 [n, 2] sorted
    distinct (query, entity) pairs with gaps), n_old, n_ent, n_scores (the size of scores_all the pairs need)."""
    rng = np.random.default_rng(900 + case.seed)
    f = lambda *shape, scale=1.0: (rng.standard_normal(shape) * scale).astype(np.float32)
    d, n = case.d, case.n
    prev_idx, n_old = _prev_runs(rng, n) if case.prev == "runs" else _prev(rng, case.prev, n)
    agg = f(n, d)
    if case.rows == "spike":
        a = agg.astype(np.float64) * 10.0 ** rng.uniform(-3, 2, (n, 1))
        r = np.arange(n)
        a[r, r % d] = 8.0 * np.abs(a).max(1) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
        agg = a.astype(np.float32)
    elif case.rows == "x_over_h":
        agg = agg * np.float32(100.0)
    elif case.rows == "h_over_x":
        agg = agg * np.float32(1e-3)
    n_ent = 37
    flat = np.sort(rng.choice(3 * n + 5, n, replace=False)).astype(np.int64)
    nodes = np.stack([flat // n_ent, flat % n_ent], 1).astype(np.int32)
    return dict(agg=agg, prev_idx=prev_idx, n_old=n_old,
                hidden_prev=None if prev_idx is None else np.clip(f(max(n_old, 1), d, scale=0.5), -1, 1),
                W_h=f(d, d, scale=d ** -0.5), w_ih=f(3 * d, d, scale=d ** -0.5), w_hh=f(3 * d, d, scale=d ** -0.5),
                b_ih=f(3 * d, scale=0.3), b_hh=f(3 * d, scale=0.3),
                Ws_next=f(case.attn_dim, d, scale=case.ws_scale * d ** -0.5) if case.attn_dim else None,
                W_final=f(d, scale=d ** -0.5) if case.readout else None, nodes=nodes, n_ent=n_ent, n_scores=3 * n + 5)


def infer_forward(case, x, dtype=np.float64, fault=None):
    return forward(x["agg"], x["hidden_prev"], x["prev_idx"], x["W_h"], case.act, x["w_ih"], x["w_hh"], x["b_ih"], x["b_hh"], None,
                   x["Ws_next"], case.ap if case.attn_dim else None, dtype=dtype, fault=fault, W_final=x["W_final"])


def infer_forward_f16x2(case, x, fault=None):
    return forward_f16x2(x["agg"], x["hidden_prev"], x["prev_idx"], x["W_h"], case.act, x["w_ih"], x["w_hh"], x["b_ih"], x["b_hh"],
                         x["Ws_next"], case.ap if case.attn_dim else None, x["W_final"], fault=fault)
