"""Reference of RDigraph.saliency: tests/rescore_ref.rescore restated in torch with a gate on every edge's message, the gradient of the
rows' scores with respect to the gates by autograd.  TEST INFRASTRUCTURE.

    agg[o] = sum over the live edges e into o of g_e * alpha_e * (hidden[s] + rela[r]),       edge_grad[e] = d score(row of e) / d g_e at g = 1

The gate multiplies the message only: alpha_e does not see g_e (it sees the gates of earlier hops through hidden[s]).  A row's score
depends on its own edges alone, so the gradient of the SUM of the scores is every row's gradient.  ``dtype`` torch.float64 is the
reference, torch.float32 the yardstick of what an fp32 evaluation costs (CPU, edges added in list order).  Nothing here is taken from
the library.
"""
import numpy as np
import torch

_ACTS = {"relu": torch.relu, "tanh": torch.tanh, "idd": lambda x: x}


def _find(keys, want):
    if len(keys) == 0:
        return np.zeros(len(want), np.int64), np.zeros(len(want), bool)
    pos = np.minimum(np.searchsorted(keys, want), len(keys) - 1)
    return pos, keys[pos] == want


def forward(p, edges, q_sub, q_rel, n_ent, L, act, keep=None, gate=None, dtype=torch.float64):
    """(score [B] torch, reached bool [B], live bool [E], alpha [E] torch) of rescore_ref.rescore with the messages multiplied by
    ``gate`` (torch [E]; None: ones).  Differentiable in ``gate``."""
    g = lambda k: torch.as_tensor(np.asarray(p[k])).to(dtype)
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    row, hop, head, rel, tail = e.T
    q_sub, q_rel = np.asarray(q_sub, np.int64), np.asarray(q_rel, np.int64)
    B, E, d = len(q_sub), len(e), g("W_final.weight").shape[1]
    keep = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    gate = torch.ones(E, dtype=dtype) if gate is None else gate
    score, reached = torch.zeros(B, dtype=dtype), np.zeros(B, bool)
    live, alpha = np.zeros(E, bool), torch.zeros(E, dtype=dtype)
    keys_prev = np.arange(B) * n_ent + q_sub
    hidden = torch.zeros((B, d), dtype=dtype)
    w_ih, w_hh, b_ih, b_hh = g("gate.weight_ih_l0"), g("gate.weight_hh_l0"), g("gate.bias_ih_l0"), g("gate.bias_hh_l0")
    for l in range(1, L + 1):
        pre = "gnn_layers.%d." % (l - 1)
        at = np.nonzero((hop == l) & keep)[0]
        src, ok = _find(keys_prev, row[at] * n_ent + head[at])
        at, src = at[ok], src[ok]
        if len(at) == 0:
            return score, reached, live, alpha
        live[at] = True
        keys, dst = np.unique(row[at] * n_ent + tail[at], return_inverse=True)
        rela = g(pre + "rela_embed.weight")
        hs, hr, hq = hidden[src], rela[rel[at]], rela[q_rel[row[at]]]
        z = hs @ g(pre + "Ws_attn.weight").T + hr @ g(pre + "Wr_attn.weight").T + hq @ g(pre + "Wqr_attn.weight").T + g(pre + "Wqr_attn.bias")
        al = torch.sigmoid(torch.relu(z) @ g(pre + "w_alpha.weight").T + g(pre + "w_alpha.bias"))
        alpha = alpha.index_put((torch.as_tensor(at),), al[:, 0].detach())
        agg = torch.zeros((len(keys), d), dtype=dtype).index_add(0, torch.as_tensor(dst.reshape(-1)), gate[at][:, None] * al * (hs + hr))
        x = _ACTS[act](agg @ g(pre + "W_h.weight").T)
        pos, had = _find(keys_prev, keys)
        h0 = torch.zeros((len(keys), d), dtype=dtype)
        h0[had] = hidden[pos[had]]
        gi, gh = x @ w_ih.T + b_ih, h0 @ w_hh.T + b_hh
        r_, z_ = torch.sigmoid(gi[:, :d] + gh[:, :d]), torch.sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
        n_ = torch.tanh(gi[:, 2 * d:] + r_ * gh[:, 2 * d:])
        hidden = (1 - z_) * n_ + z_ * h0
        keys_prev = keys
    rows = keys_prev // n_ent
    assert len(np.unique(rows)) == len(rows), "the hop-L edges of a row must share their tail"
    score = score.index_put((torch.as_tensor(rows),), (hidden @ g("W_final.weight").T)[:, 0])
    reached[rows] = True
    return score, reached, live, alpha


def saliency(p, edges, q_sub, q_rel, n_ent, L, act, keep=None, dtype=torch.float64):
    """(score [B], reached bool [B], live bool [E], alpha [E], edge_grad [E]) in numpy: forward at gate = 1 and the gradient of the
    summed scores with respect to the gates."""
    E = len(np.asarray(edges).reshape(-1, 5))
    gate = torch.ones(E, dtype=dtype, requires_grad=True)
    score, reached, live, alpha = forward(p, edges, q_sub, q_rel, n_ent, L, act, keep, gate, dtype)
    grad = torch.autograd.grad(score.sum(), gate)[0] if score.requires_grad else torch.zeros(E, dtype=dtype)
    return score.detach().numpy(), reached, live, alpha.numpy(), grad.numpy()


def finite_differences(p, edges, q_sub, q_rel, n_ent, L, act, keep, live, step=1e-6):
    """Central differences of the fp64 scores in the gate of every live edge, [E] (0 elsewhere).  A row's score depends on its own
    edges only, so the j-th live edge of EVERY row is moved in one pair of forwards."""
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
                gate = torch.ones(E, dtype=torch.float64)
                gate[at] += sign * step
                side.append(forward(p, edges, q_sub, q_rel, n_ent, L, act, keep, gate)[0].numpy()[rows])
            out[at] = (side[0] - side[1]) / (2 * step)
    return out
