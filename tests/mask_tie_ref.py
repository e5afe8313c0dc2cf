"""Reference of tied edge masks: the grouping of explain.mask_groups, the defined sum of rg_mask_tie_grad and learn_mask(tie=)'s loop.
TEST INFRASTRUCTURE; nothing here is taken from the library.

``groups`` is the grouping in plain Python on the (row, hop, head, rel, tail) rows: a dict keyed by (row, key...) of the free edges'
positions, the keys sorted, the positions ascending.

``group_sums32`` is include/redgnn.h's definition of the sum, one np.float32 addition at a time: a group is cut into chunks of
``chunk`` members counted from its own first member, a chunk's sum starts from its first member's value and adds the rest in member
order, a group's sum is its chunk sums added in chunk order starting from the first, and an empty group gives +0.  ``group_sums64``
is the same sum in fp64 (where the order no longer matters at the tolerance).

``learn_tied`` is tests/mask_ref.learn's loop with the tie: ig_ref.gradient_at's gradient summed per group, mask_ref.step on the
group cells, the groups' gates copied to their edges."""
import types

import numpy as np

from tests import mask_ref as MR


def groups(edges, n_rel, tie, free):
    """namespace(group_of int32 [E], grp_ptr int32 [G + 1], member int32 [M], row_ptr int64 [B'] over the rows up to the largest one
    that has a group, group_row int64 [G], group_key int64 [G, c]) of the edges ``free``; ``tie``: "fact", "relation" or int labels [E]."""
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    free = np.asarray(free).astype(bool)
    table = {}
    for pos, (row, hop, h, r, t) in enumerate(e.tolist()):
        if not free[pos]:
            continue
        if isinstance(tie, str) and tie == "fact":
            if r == 2 * n_rel:
                continue
            key = (h, r, t) if r < n_rel else (t, r - n_rel, h)
        elif isinstance(tie, str) and tie == "relation":
            key = (hop, r)
        else:
            key = (int(np.asarray(tie)[pos]),)
        table.setdefault((row,) + key, []).append(pos)
    keys = sorted(table)
    group_of = np.full(len(e), -1, np.int32)
    grp_ptr, member = [0], []
    for g, key in enumerate(keys):
        group_of[table[key]] = g
        member += table[key]
        grp_ptr.append(len(member))
    c = {"fact": 3, "relation": 2}.get(tie, 1) if isinstance(tie, str) else 1
    k = np.array(keys, np.int64).reshape(-1, 1 + c)
    return types.SimpleNamespace(group_of=group_of, grp_ptr=np.array(grp_ptr, np.int32), member=np.array(member, np.int32),
                                 group_row=k[:, 0], group_key=k[:, 1:], n_groups=len(keys))


def row_ptr(group_row, B):
    out = np.zeros(B + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(group_row, minlength=B)[:B])
    return out


def group_sums32(grp_ptr, member, grad, chunk=32):
    """float32 [R, G]: the defined sum, every addition rounded to float32."""
    grad = np.asarray(grad, np.float32)
    R, G = grad.shape[0], len(grp_ptr) - 1
    out = np.zeros((R, G), np.float32)
    for k in range(R):
        for g in range(G):
            lo, hi = int(grp_ptr[g]), int(grp_ptr[g + 1])
            total = None
            for c0 in range(lo, hi, chunk):
                acc = grad[k, member[c0]]
                for p in range(c0 + 1, min(c0 + chunk, hi)):
                    acc = np.float32(acc + grad[k, member[p]])
                total = acc if total is None else np.float32(total + acc)
            if total is not None:
                out[k, g] = total
    return out


def group_sums64(grp_ptr, member, grad):
    """float64 [R, G]: the same sums in fp64."""
    grad = np.asarray(grad, np.float64)
    return np.stack([np.array([grad[k, member[grp_ptr[g]:grp_ptr[g + 1]]].sum() for g in range(len(grp_ptr) - 1)], np.float64)
                     for k in range(grad.shape[0])]).reshape(grad.shape[0], len(grp_ptr) - 1)


def learn_tied(p, edges, q_sub, q_rel, n_ent, n_rel, L, act, lam, entropy, iterations, lr, theta0, tie, keep=None, dtype=np.float64):
    """mask_ref.learn with the tie, for ONE lambda: dict(target, baseline_score, scale, inv_scale, free [E], groups (the namespace of
    ``groups``), n_groups [B], group_grad [iterations, G] = the group gradient at the gates iteration i starts from, group_gate [G] and
    gate [E] after the loop, deviation / size / count [iterations, B], reached)."""
    import torch
    from tests import ig_ref as IG
    tdt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    e = np.asarray(edges, np.int64).reshape(-1, 5)
    E, B = len(e), len(q_sub)
    kept = np.ones(E, bool) if keep is None else np.asarray(keep).astype(bool)
    fixed = kept & (e[:, 3] == 2 * n_rel)
    free = kept & ~fixed
    T = groups(e, n_rel, tie, free)
    G = T.n_groups
    offsets = row_ptr(T.group_row, B)
    at = lambda gate: IG.gradient_at(p, e, q_sub, q_rel, n_ent, L, act, gate, keep, dtype=tdt)
    target, reached = at(np.ones(E))[:2]
    baseline = at(fixed.astype(np.float64))[0]
    scale = np.abs(target - baseline)
    inv_scale = np.where((scale > 0) & reached, 1.0 / np.where(scale > 0, scale, 1.0), 0.0).astype(dtype)
    n_groups = np.diff(offsets)
    inv_n = np.where(n_groups > 0, 1.0 / np.maximum(n_groups, 1), 0.0)
    theta, m, v = np.full((1, G), float(theta0)), np.zeros((1, G)), np.zeros((1, G))
    g0 = 1.0 / (1.0 + np.exp(-float(theta0)))
    grp_gate = np.full((1, G), g0)
    gate = np.where(free, g0, fixed.astype(np.float64))
    out = dict(deviation=np.zeros((iterations, B)), size=np.zeros((iterations, B)), count=np.zeros((iterations, B), np.int64),
               group_grad=np.zeros((iterations, G)))
    for it in range(iterations):
        score, _, _, _, grad = at(gate)
        out["deviation"][it] = (score - target) * inv_scale
        gg = (group_sums64 if np.dtype(dtype) == np.float64 else group_sums32)(T.grp_ptr, T.member, grad[None, :])
        out["group_grad"][it] = gg[0]
        s = MR.step(offsets, np.ones(G, bool), score[None, :], target, inv_scale, inv_n, [lam], [entropy], gg, theta, m, v, it + 1, lr,
                    dtype=dtype, gate_in=grp_gate)
        theta, m, v, grp_gate = s["theta"], s["m"], s["v"], s["gate"]
        gate = np.where(T.group_of >= 0, np.asarray(grp_gate[0], np.float64)[np.maximum(T.group_of, 0)], gate)
        out["size"][it], out["count"][it] = s["size"][0], s["count"][0]
    return dict(out, target=target, baseline_score=baseline, scale=scale, inv_scale=inv_scale, free=free, groups=T, n_groups=n_groups,
                group_gate=np.asarray(grp_gate[0]), gate=gate, reached=reached)
