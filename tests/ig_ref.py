"""Reference of RDigraph.integrated_gradients: tests/saliency_ref.forward - rescore_ref's forward in torch with a gate on every edge's
message - under the midpoint rule along the straight path of gates from a baseline to a target.  TEST INFRASTRUCTURE.

    t_k = (k + 1/2) / steps,  gate_k = lo + t_k (hi - lo),  edge_attr = sum_k (1 / steps) (hi - lo) d score / d gate at gate_k   (k ascending)
    residual[b] = score(hi)[b] - score(lo)[b] - the sum of row b's edge_attr

The default baseline holds the identity edges (relation 2 n_rel) at 1 and every other edge at 0, the default target is 1 everywhere.
``dtype`` torch.float64 is the reference, torch.float32 the yardstick of what an fp32 evaluation costs.  Nothing here is taken from the
library.
"""
import numpy as np
import torch

from tests import saliency_ref as S


def default_baseline(edges, n_rel):
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    return (e[:, 3] == 2 * n_rel).astype(np.float64)


def gradient_at(p, edges, q_sub, q_rel, n_ent, L, act, gate, keep=None, dtype=torch.float64):
    """(score [B], reached, live, alpha [E], edge_grad [E]) in numpy at the gates ``gate`` [E]: saliency_ref.saliency anywhere but at 1."""
    g = torch.as_tensor(np.asarray(gate)).to(dtype).clone().requires_grad_(True)
    score, reached, live, alpha = S.forward(p, edges, q_sub, q_rel, n_ent, L, act, keep, g, dtype)
    grad = torch.autograd.grad(score.sum(), g)[0] if score.requires_grad else torch.zeros_like(g)
    return score.detach().numpy(), reached, live, alpha.numpy(), grad.detach().numpy()


def finite_differences_at(p, edges, q_sub, q_rel, n_ent, L, act, gate, keep, live, step=1e-6):
    """Central differences of the fp64 scores in the gate of every live edge around ``gate``, [E] (0 elsewhere): saliency_ref's, which
    moves the j-th live edge of every row in one pair of forwards, at any gate."""
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    B, E = len(q_sub), len(e)
    out = np.zeros(E)
    per_row = [np.nonzero(live & (e[:, 0] == b))[0] for b in range(B)]
    with torch.no_grad():
        for j in range(max((len(x) for x in per_row), default=0)):
            rows = np.array([b for b in range(B) if j < len(per_row[b])])
            at = np.array([per_row[b][j] for b in rows])
            side = []
            for sign in (1.0, -1.0):
                g = torch.as_tensor(np.asarray(gate, np.float64)).clone()
                g[at] += sign * step
                side.append(S.forward(p, edges, q_sub, q_rel, n_ent, L, act, keep, g)[0].numpy()[rows])
            out[at] = (side[0] - side[1]) / (2 * step)
    return out


def integrated_gradients(p, edges, q_sub, q_rel, n_ent, n_rel, L, act, steps, keep=None, baseline=None, target=None, dtype=torch.float64):
    """dict(score, baseline_score, edge_attr, residual [numpy, in ``dtype``], reached, live) of the midpoint rule with ``steps`` steps."""
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    E, B = len(e), len(q_sub)
    lo = torch.as_tensor(default_baseline(e, n_rel) if baseline is None else np.asarray(baseline)).to(dtype)
    hi = torch.ones(E, dtype=dtype) if target is None else torch.as_tensor(np.asarray(target)).to(dtype)
    with torch.no_grad():
        score, reached, live, _ = S.forward(p, e, q_sub, q_rel, n_ent, L, act, keep, hi, dtype)
        base = S.forward(p, e, q_sub, q_rel, n_ent, L, act, keep, lo, dtype)[0]
    attr = torch.zeros(E, dtype=dtype)
    weight = (hi - lo) * torch.tensor(1.0 / steps, dtype=dtype)
    for k in range(steps):
        t = torch.tensor((k + 0.5) / steps, dtype=dtype)
        grad = gradient_at(p, e, q_sub, q_rel, n_ent, L, act, lo + t * (hi - lo), keep, dtype)[4]
        attr = attr + weight * torch.as_tensor(grad)
    attr = torch.where(hi != lo, attr, torch.zeros_like(attr))
    sums = torch.zeros(B, dtype=dtype).index_add(0, torch.as_tensor(e[:, 0]), attr)
    return dict(score=score.numpy(), baseline_score=base.numpy(), edge_attr=attr.numpy(), residual=(score - base - sums).numpy(),
                reached=reached, live=live)
