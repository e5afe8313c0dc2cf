"""Per-edge reference of rg_digraph_layer_fwd_gated and rg_digraph_layer_bwd_gated - one edge-list hop and its adjoint with a gate on
every edge's message, for n_rep replicas of the hop - in plain numpy, fp64 and fp32, on the arithmetic of tests/layer_ref.py and the
cases of tests/digraph_bwd_ref.py.  TEST INFRASTRUCTURE.

Replica k has its own hidden, a_s and grad_agg rows (k * n_src + s, k * n_dst + o) and the gate

    g_e = fmaf(t[k], gate_hi[e] - gate_lo[e], gate_lo[e])                      an fp32 value: include/redgnn.h defines it so

``gate_of`` forms that float (the difference rounded to fp32, then the fused multiply-add rounded once: the product of two fp32 values
and its sum with a third are exact in fp64 up to the final rounding).  The reference takes it as given, in fp64, so the gate's own
rounding is part of the input and not of the error.  Per edge e = (b, s, r, o), G = grad_agg, m = hidden[s] + rela[r]:

    agg[o]          += g alpha m                      S: |g| kappa |m|                          n0 = layer_ref's + 1
    grad_gate[e]     = alpha <G[o], m>                S, n, n0: digraph_bwd_ref's, unchanged: the gate does not scale it
    grad_hidden[s]  += g alpha G[o]                   S: |g| kappa |G|                          n0 = layer_ref's + 1
    grad_a_s[s]     += g g_alpha alpha (1 - alpha) w 1[pre > 0]     S: |g| times layer_ref's    n0 = layer_ref's + 1

layer_ref's error model as it stands (kappa, U, C_BOUND), every gated term's magnitude scaled by |g| and one more rounding per term
(the product c = g * alpha, or g * g_p).
"""
import types

import numpy as np

from tests import digraph_bwd_ref as D
from tests import layer_ref as lr

T = np.array([0.0, 0.37, 1.0], np.float32)                 # the replicas of every case
FWD_OUTPUTS = ("agg",)
BWD_OUTPUTS = D.OUTPUTS


def n0_of(name, d, attn_dim):
    if name == "grad_gate":
        return D.n0_of(name, d, attn_dim)
    return lr.n0_of(name, d, attn_dim) + 1


def gate_of(t, lo, hi, E):
    """float32 [E]: fmaf(t, hi - lo, lo) as the kernels form it (lo / hi None: 0 / 1)."""
    lo = np.zeros(E, np.float32) if lo is None else np.asarray(lo, np.float32)
    hi = np.ones(E, np.float32) if hi is None else np.asarray(hi, np.float32)
    diff = (hi - lo).astype(np.float32)
    return (np.float64(np.float32(t)) * diff.astype(np.float64) + lo.astype(np.float64)).astype(np.float32)


def gates(E, seed):
    """(gate_lo, gate_hi) float32 [E]: random, with an exact 0, an exact 1, a negative value and a value above 1 in each, at different
    places (as many of them as E has room for)."""
    rng = np.random.default_rng(900 + seed)
    lo, hi = rng.uniform(-0.5, 1.5, E).astype(np.float32), rng.uniform(-0.5, 1.5, E).astype(np.float32)
    special = np.array([0.0, 1.0, -0.75, 1.625], np.float32)
    at = rng.permutation(E)[:4]
    lo[at] = special[:len(at)]
    hi[at[::-1]] = special[:len(at)]
    return lo, hi


def replica_inputs(c, k, hop, n_rep):
    """layer_ref.inputs for ``n_rep`` replicas: hidden [n_rep * n_old, ld], a_s [n_rep * n_old, ap] and grad_agg [n_rep * n_new, ld] with
    a block of their own per replica (replica 0: layer_ref.inputs' own), the other tables shared."""
    x = lr.inputs(c, k, hop)
    own = {name: [x[name]] for name in ("hidden", "a_s", "grad_agg")}
    for j in range(1, n_rep):
        other = lr.inputs(types.SimpleNamespace(**{**vars(c), "seed": c.seed + 1000 * j}), k, hop)
        for name in own:
            own[name].append(other[name])
    return dict(x, **{name: np.concatenate(v, 0) for name, v in own.items()})


def _replica(x, hop, j):
    rows = lambda a, n: a[j * n:(j + 1) * n]
    return dict(x, hidden=rows(x["hidden"], hop.n_old), a_s=rows(x["a_s"], hop.n_old), grad_agg=rows(x["grad_agg"], hop.n_new))


def _forward_one(hop, x, g, dtype):
    dt = np.dtype(dtype)
    keys = ("hidden", "rela", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")
    h, r, as_, ar, aq, w, b = lr._cast(dt, *(x[k] for k in keys))
    _, _, alpha = lr._attention(hop, as_, ar, aq, w, b)
    agg = lr._scatter(hop.o, (g.astype(dt) * alpha)[:, None] * lr._message(hop, h, r, None), hop.n_new)
    h, r, as_, ar, aq, w, b = lr._cast(np.float64, *(x[k] for k in keys))
    _, _, a64 = lr._attention(hop, as_, ar, aq, w, b)
    S = lr._scatter(hop.o, (np.abs(g.astype(np.float64)) * lr._kappa(hop, as_, ar, aq, w, b, a64))[:, None]
                    * lr._message(hop, h, r, None, absolute=True), hop.n_new)
    return agg, alpha, S


def forward(hop, x, t, lo, hi, dtype=np.float64):
    """agg [n_rep * n_new, ld], alpha [n_rep * E] in ``dtype``; .S / .n per output, stacked like the outputs."""
    parts = [_forward_one(hop, _replica(x, hop, j), gate_of(tj, lo, hi, hop.E), dtype) for j, tj in enumerate(t)]
    n = np.tile(np.bincount(hop.o, minlength=hop.n_new)[:, None], (len(t), 1))
    return types.SimpleNamespace(agg=np.concatenate([p[0] for p in parts], 0), alpha=np.concatenate([p[1] for p in parts]),
                                 S=dict(agg=np.concatenate([p[2] for p in parts], 0)), n=dict(agg=n))


def _backward_values(hop, x, g, dt, absolute):
    keys = ("hidden", "rela", "a_s", "a_r", "a_q", "w_alpha", "b_alpha", "grad_agg")
    h, r, as_, ar, aq, w_alpha, b, G_rows = lr._cast(dt, *(x[k] for k in keys))
    w, zr, alpha = lr._attention(hop, as_, ar, aq, w_alpha, b)
    G, g = G_rows[hop.o], g.astype(dt)
    if absolute:
        G, w, g = np.abs(G), np.abs(w), np.abs(g)
        alpha = lr._kappa(hop, as_, ar, aq, w_alpha, b, alpha)
    m = lr._message(hop, h, r, None, absolute)
    g_alpha = (G * m).sum(1, dtype=G.dtype)
    g_p = g_alpha * alpha if absolute else g_alpha * alpha * (G.dtype.type(1) - alpha)
    g_z = (g * g_p)[:, None] * w[None, :] * (zr > 0)
    return dict(grad_gate=alpha * g_alpha, grad_hidden=lr._scatter(hop.hrow, (g * alpha)[:, None] * G, hop.n_old),
                grad_a_s=lr._scatter(hop.s, g_z, hop.n_old))


def backward(hop, x, t, lo, hi, dtype=np.float64):
    """grad_gate [n_rep * E], grad_hidden [n_rep * n_old, ld], grad_a_s [n_rep * n_old, ap] in ``dtype``; .S / .n per output."""
    vals, S = [], []
    for j, tj in enumerate(t):
        xj, g = _replica(x, hop, j), gate_of(tj, lo, hi, hop.E)
        vals.append(_backward_values(hop, xj, g, np.dtype(dtype), False))
        S.append(_backward_values(hop, xj, g, np.dtype(np.float64), True))
    cat = lambda parts, name: np.concatenate([p[name] for p in parts], 0)
    cnt = np.tile(np.bincount(hop.s, minlength=hop.n_old)[:, None], (len(t), 1))
    return types.SimpleNamespace(S={k: cat(S, k) for k in BWD_OUTPUTS}, n=dict(grad_gate=np.ones(len(t) * hop.E), grad_hidden=cnt, grad_a_s=cnt),
                                 **{k: cat(vals, k) for k in BWD_OUTPUTS})


def all_hops():
    """Every (tag, case, k, hop, A) the gated kernels' tests use: digraph_bwd_ref's."""
    return D.all_hops()
