"""Reference of RDigraph.saliency for the two temporal models: tests/trescore_ref.rescore (interpolation) and tests/xrescore_ref.rescore
(extrapolation) restated in torch with a gate on every edge's message, the gradient of the rows' scores with respect to the gates by
autograd.  TEST INFRASTRUCTURE.

    agg[o] = sum over the live edges e into o of g_e * alpha_e * W_dir(e) (hidden[s] + rela[r] + time embedding(e))
    edge_grad[e] = d score(row of e) / d g_e at g = 1

W_dir(e) is the Linear of the edge's direction (interpolation: past / now / future of edge time - query time) or past_linear
(extrapolation).  The gate multiplies the message only: alpha_e does not see g_e (it sees the gates of earlier hops through
hidden[s]).  Neither model has a GRU: the new state is act(agg).  A row's score depends on its own edges alone, so the gradient of
the SUM of the scores is every row's gradient.  ``dtype`` torch.float64 is the reference, torch.float32 the yardstick of what an fp32
evaluation costs (CPU, edges added in list order).  Nothing here is taken from the library.
"""
import numpy as np
import torch

from tests.saliency_ref import _find

_ACTS = {"relu": torch.relu, "tanh": torch.tanh, "idd": lambda x: x}


def _param(p, dtype):
    return lambda k: torch.as_tensor(np.asarray(p[k].detach().cpu().numpy() if hasattr(p[k], "detach") else p[k])).to(dtype)


def _periodic(g, lag):
    """tests/extrap_ref.periodic_embedding in torch: lag [N] -> [N, d]."""
    x = lag.reshape(-1, 1)
    z = 2 * np.pi * g("time_embed.periodic.weight") * x
    z = torch.cat([torch.cos(z), torch.sin(z)], 1)
    neg = z @ g("time_embed.linear_neg.weight")[0] + g("time_embed.linear_neg.bias")
    pos = z @ g("time_embed.linear_pos.weight")[0] + g("time_embed.linear_pos.bias")
    return torch.relu(torch.where(x < 0, neg, pos))


def forward(kind, p, edges, time, q_time, heads, rels, n_ent, L, act, keep=None, gate=None, shared_tables=False, dtype=torch.float64):
    """(score [B] torch, reached bool [B], live bool [E], alpha [E] torch) of trescore_ref.rescore (``kind`` "temporal": ``time`` the
    edges' time ids, ``q_time`` the rows') or xrescore_ref.rescore ("extrapolation": the edges' days and the rows' query days) with
    the messages multiplied by ``gate`` (torch [E]; None: ones).  Differentiable in ``gate``."""
    g = _param(p, dtype)
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    row, hop, head, rel, tail = e.T
    time, q_time = np.asarray(time, np.int64), np.asarray(q_time, np.int64).reshape(-1)
    heads, rels = np.asarray(heads, np.int64).reshape(-1), np.asarray(rels, np.int64).reshape(-1)
    if kind == "temporal":
        W = [g("past_linear.weight"), g("now_linear.weight"), g("future_linear.weight")]       # by direction 0 / 1 / 2
        temb = g("time_embed.weight")
    else:
        W = [g("past_linear.weight")]
    B, E, d = len(heads), len(e), W[0].shape[0]
    keep = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    gate = torch.ones(E, dtype=dtype) if gate is None else gate
    score, reached = torch.zeros(B, dtype=dtype), np.zeros(B, bool)
    live, alpha = np.zeros(E, bool), torch.zeros(E, dtype=dtype)
    keys_prev = np.arange(B) * n_ent + heads
    hidden = torch.zeros((B, d), dtype=dtype)
    for l in range(1, L + 1):
        if shared_tables:
            rela, w1, w2 = g("rela_embed.weight"), g("attention_1.weight"), g("attention_2.weight")
        else:
            rela, w1, w2 = (g("%s.%d.weight" % (name, l - 1)) for name in ("rela_embed_layer", "attention_1_layer", "attention_2_layer"))
        at = np.nonzero((hop == l) & keep)[0]
        src, ok = _find(keys_prev, row[at] * n_ent + head[at])
        at, src = at[ok], src[ok]
        if len(at) == 0:
            return score, reached, live, alpha
        live[at] = True
        keys, dst = np.unique(row[at] * n_ent + tail[at], return_inverse=True)
        hs, hr = hidden[src], rela[rel[at]]
        if kind == "temporal":
            dt = time[at] - q_time[row[at]]
            d_of = np.where(dt > 0, 2, np.where(dt == 0, 1, 0))
            embed = hs + hr + temb[np.abs(dt)]
            msg = torch.zeros_like(embed)
            for k in range(3):
                sel = torch.as_tensor(np.nonzero(d_of == k)[0])
                msg = msg.index_add(0, sel, embed[sel] @ W[k].T)
        else:
            lag = torch.as_tensor((q_time[row[at]] - time[at]).astype(np.float64)).to(dtype)
            msg = (hs + hr + _periodic(g, lag)) @ W[0].T
        att_in = torch.cat([hs, hr, rela[rels[row[at]]]], 1)
        al = torch.sigmoid(torch.relu(att_in @ w1.T) @ w2.T)
        alpha = alpha.index_put((torch.as_tensor(at),), al[:, 0].detach())
        agg = torch.zeros((len(keys), d), dtype=dtype).index_add(0, torch.as_tensor(dst.reshape(-1)), gate[at][:, None] * al * msg)
        hidden = _ACTS[act](agg)
        keys_prev = keys
    rows = keys_prev // n_ent
    assert len(np.unique(rows)) == len(rows), "the hop-L edges of a row must share their tail"
    score = score.index_put((torch.as_tensor(rows),), (hidden @ g("linear_classifier.weight").T + g("linear_classifier.bias"))[:, 0])
    reached[rows] = True
    return score, reached, live, alpha


def saliency(kind, p, edges, time, q_time, heads, rels, n_ent, L, act, keep=None, shared_tables=False, dtype=torch.float64):
    """(score [B], reached bool [B], live bool [E], alpha [E], edge_grad [E]) in numpy: forward at gate = 1 and the gradient of the
    summed scores with respect to the gates."""
    E = len(np.asarray(edges).reshape(-1, 5))
    gate = torch.ones(E, dtype=dtype, requires_grad=True)
    score, reached, live, alpha = forward(kind, p, edges, time, q_time, heads, rels, n_ent, L, act, keep, gate, shared_tables, dtype)
    grad = torch.autograd.grad(score.sum(), gate)[0] if score.requires_grad else torch.zeros(E, dtype=dtype)
    return score.detach().numpy(), reached, live, alpha.numpy(), grad.numpy()


def finite_differences(kind, p, edges, time, q_time, heads, rels, n_ent, L, act, keep, live, shared_tables=False, step=1e-6, most=None):
    """Central differences of the fp64 scores in the gate of the live edges, [E] (0 elsewhere; ``most``: only the first ``most`` live
    edges of every row, the others NaN).  A row's score depends on its own edges only, so the j-th live edge of EVERY row is moved in
    one pair of forwards."""
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    B, E = len(heads), len(e)
    out = np.zeros(E)
    per_row = [np.nonzero(live & (e[:, 0] == b))[0] for b in range(B)]
    if most is not None:
        for x in per_row:
            out[x[most:]] = np.nan
        per_row = [x[:most] for x in per_row]
    with torch.no_grad():
        for j in range(max((len(x) for x in per_row), default=0)):
            rows = np.array([b for b in range(B) if j < len(per_row[b])])
            at = np.array([per_row[b][j] for b in rows])
            side = []
            for sign in (1.0, -1.0):
                gate = torch.ones(E, dtype=torch.float64)
                gate[at] += sign * step
                side.append(forward(kind, p, edges, time, q_time, heads, rels, n_ent, L, act, keep, gate, shared_tables)[0].numpy()[rows])
            out[at] = (side[0] - side[1]) / (2 * step)
    return out
