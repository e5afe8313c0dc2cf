"""Reference of rg_mask_step and of RDigraph.learn_mask's loop.  TEST INFRASTRUCTURE; nothing here is taken from the library.

``step`` is one update of include/redgnn.h's rg_mask_step in plain numpy for a given dtype - np.float64 is the reference, np.float32
the yardstick of what an fp32 evaluation of the same formulas costs:

    g = 1 / (1 + exp(-theta));  coef = 2 (score - target) inv_scale^2
    dL/dg = coef grad + lambda_size inv_n - lambda_ent theta;   gt = dL/dg g (1 - g)
    m' = b1 m + (1 - b1) gt;  v' = b2 v + (1 - b2) gt^2;  theta' = theta - lr (m' / (1 - b1^t)) / (sqrt(v' / (1 - b2^t)) + eps)
    gate = 1 / (1 + exp(-theta'))

on the free edges, everything else left as it is; size / count per (replica, row) over the row's free edges.

``make_inputs`` draws inputs away from Adam's first-step sign sensitivity: at step 1 from zero moments the update is lr * sign(gt)
(m' / sqrt(v') = +-1), so a gt that rounding can carry through 0 flips theta' by 2 lr.  With both lambdas 0, |grad| in [0.1, 3] and
|score - target| >= 0.25, gt keeps its sign in every precision.

``learn`` is the driver's loop in torch, fp64, on tests/ig_ref.gradient_at, one replica (one lambda) at a time."""
import types

import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def _row_of(offsets, E):
    return np.repeat(np.arange(len(offsets) - 1), np.diff(np.asarray(offsets, np.int64)))[:E]


def step(offsets, free, score, target, inv_scale, inv_n, lambda_size, lambda_ent, grad, theta, m, v, t, lr, dtype=np.float64,
         beta1=BETA1, beta2=BETA2, eps=EPS, gate_in=None):
    """One step for R replicas: dict(theta, m, v, gate [R, E], size [R, B] in ``dtype``, count int [R, B]).  ``gate_in`` [R, E]: what
    the gate array holds where an edge is not free (default 0)."""
    dt = np.dtype(dtype).type
    c = lambda x: np.asarray(x, dtype=np.float64).astype(dtype)
    free = np.asarray(free).astype(bool)
    R, E = np.asarray(theta).shape
    B = len(offsets) - 1
    row = _row_of(offsets, E)
    score, target, inv_scale, inv_n, lam_s, lam_e = c(score), c(target), c(inv_scale), c(inv_n), c(lambda_size), c(lambda_ent)
    grad, theta0, m0, v0 = c(grad), c(theta), c(m), c(v)
    one, two = dt(1), dt(2)
    b1, b2, lr_, eps_ = dt(beta1), dt(beta2), dt(lr), dt(eps)
    bc1, bc2 = dt(1.0 - float(beta1) ** t), dt(1.0 - float(beta2) ** t)
    g = one / (one + np.exp(-theta0))
    coef = two * (score - target[None, :]) * inv_scale[None, :] * inv_scale[None, :]                # [R, B]
    dl = coef[:, row] * grad + (lam_s[:, None] * inv_n[None, :])[:, row] - lam_e[:, None] * theta0
    gt = dl * (g * (one - g))
    m1 = b1 * m0 + (one - b1) * gt
    v1 = b2 * v0 + (one - b2) * (gt * gt)
    th1 = theta0 - lr_ * (m1 / bc1) / (np.sqrt(v1 / bc2) + eps_)
    g1 = one / (one + np.exp(-th1))
    keep = lambda new, old: np.where(free[None, :], new, old)
    gate = keep(g1, np.zeros((R, E), dtype) if gate_in is None else c(gate_in))
    size, count = np.zeros((R, B), dtype), np.zeros((R, B), np.int64)
    for k in range(R):
        size[k] = np.bincount(row[free], weights=g1[k, free].astype(np.float64), minlength=B)[:B].astype(dtype)
        count[k] = np.bincount(row[free], weights=(g1[k, free] > dt(0.5)), minlength=B)[:B]
    return dict(theta=keep(th1, theta0), m=keep(m1, m0), v=keep(v1, v0), gate=gate, size=size, count=count)


def make_inputs(lengths, R, seed, free_fraction=0.8):
    """Inputs of a first step from zero moments with both lambdas 0 (see the docstring above), fp32 arrays: a namespace of offsets,
    free, score, target, inv_scale, inv_n, grad, theta and the lambdas a second step takes (lambda_size2 / lambda_ent2)."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, np.int64)
    B, E = len(lengths), int(lengths.sum())
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(lengths)
    row = _row_of(offsets, E)
    free = rng.random(E) < free_fraction
    n_free = np.bincount(row[free], minlength=B)[:B]
    f32 = lambda x: np.asarray(x, np.float32)
    target = f32(rng.uniform(-2, 2, B))
    dev = rng.uniform(0.25, 1.5, (R, B)) * rng.choice([-1.0, 1.0], (R, B))
    score = f32(target[None, :] + dev)
    score = np.where(np.abs(score.astype(np.float64) - target[None, :]) >= 0.25, score, f32(target[None, :] + 0.5))
    grad = f32(rng.uniform(0.1, 3.0, (R, E)) * rng.choice([-1.0, 1.0], (R, E)))
    return types.SimpleNamespace(
        B=B, E=E, R=R, offsets=offsets, free=free, row=row, n_free=n_free, target=target, score=f32(score),
        inv_scale=f32(1.0 / rng.uniform(0.5, 2.0, B)), inv_n=f32(np.where(n_free > 0, 1.0 / np.maximum(n_free, 1), 0.0)), grad=grad,
        theta=f32(rng.uniform(-2.5, 2.5, (R, E))), zeros=np.zeros((R, E), np.float32), lambda0=np.zeros(R, np.float32),
        lambda_size2=f32(rng.uniform(0.01, 1.0, R)), lambda_ent2=f32(rng.uniform(0.0, 0.2, R)),
        grad2=f32(rng.uniform(0.1, 3.0, (R, E)) * rng.choice([-1.0, 1.0], (R, E))),
        score2=f32(target[None, :] + rng.uniform(0.25, 1.5, (R, B)) * rng.choice([-1.0, 1.0], (R, B))))


def learn(p, edges, q_sub, q_rel, n_ent, n_rel, L, act, lam, entropy, iterations, lr, theta0, keep=None, dtype=np.float64):
    """The driver's loop in ``dtype`` (np.float64: the reference; np.float32: the yardstick) for ONE lambda: dict(target,
    baseline_score, scale, inv_scale, n_free [B], free [E], gate [E] after the loop, deviation [iterations, B], size [iterations, B],
    count [iterations, B])."""
    import torch
    from tests import ig_ref as IG
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    E, B = len(e), len(q_sub)
    kept = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    fixed = kept & (e[:, 3] == 2 * n_rel)
    free = kept & ~fixed
    offsets = np.zeros(B + 1, np.int64)
    offsets[1:] = np.cumsum(np.bincount(e[:, 0], minlength=B))
    at = lambda gate: IG.gradient_at(p, e, q_sub, q_rel, n_ent, L, act, gate, keep, dtype=tdt)
    target, reached = at(np.ones(E))[:2]
    baseline = at(fixed.astype(np.float64))[0]
    scale = np.abs(target - baseline)
    inv_scale = np.where((scale > 0) & reached, 1.0 / np.where(scale > 0, scale, 1.0), 0.0).astype(dtype)
    n_free = np.bincount(e[free, 0], minlength=B)[:B]
    inv_n = np.where(n_free > 0, 1.0 / np.maximum(n_free, 1), 0.0)
    theta, m, v = np.full((1, E), float(theta0)), np.zeros((1, E)), np.zeros((1, E))
    gate = np.where(free, 1.0 / (1.0 + np.exp(-float(theta0))), fixed.astype(np.float64))[None, :]
    out = dict(deviation=np.zeros((iterations, B)), size=np.zeros((iterations, B)), count=np.zeros((iterations, B), np.int64))
    for it in range(iterations):
        score, _, _, _, grad = at(gate[0])
        out["deviation"][it] = (score - target) * inv_scale
        s = step(offsets, free, score[None, :], target, inv_scale, inv_n, [lam], [entropy], grad[None, :], theta, m, v, it + 1, lr,
                 dtype=dtype, gate_in=gate)
        theta, m, v, gate = s["theta"], s["m"], s["v"], s["gate"]
        out["size"][it], out["count"][it] = s["size"][0], s["count"][0]
    return dict(out, target=target, baseline_score=baseline, scale=scale, inv_scale=inv_scale, n_free=n_free, free=free, gate=gate[0],
                reached=reached)
