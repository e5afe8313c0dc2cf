"""Numpy reference of rg_segment_eval: it BUILDS the dense fp32 score row of every query (the pairs' scores, +0.0 elsewhere) and works
from it - logp in float64, the six counts by direct comparison under keep-masks - plus the literal torch sequence of the reference's
validation loop (Temporal/interpolation/main.py:142-164, util.py:42-51) for the host test."""
import numpy as np


def dense_row(scores, ent, n_ent):
    x = np.zeros(n_ent, np.float32)
    x[np.asarray(ent, dtype=np.int64)] = np.asarray(scores, dtype=np.float32)
    return x


def list_of(index, key):
    """The list of ``key`` in a (keys, ptr, idx) index, empty when the index is None or lacks the key."""
    if index is None:
        return np.zeros(0, np.int64)
    keys, ptr, idx = (np.asarray(a) for a in index)
    i = np.searchsorted(keys, key)
    if i < len(keys) and keys[i] == key:
        return idx[ptr[i]:ptr[i + 1]].astype(np.int64)
    return np.zeros(0, np.int64)


def row_eval(x, t, list_a=(), list_b=()):
    """(logp float64, counts int64 [6], visited is not known from the row) of target t on the dense row x (fp32)."""
    n_ent = len(x)
    x64 = x.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if np.isnan(x64).any():
            logp = np.nan
        else:
            m = x64.max()
            ex = np.exp(x64 - m)
            logp = np.log(ex[t] / ex.sum() + 1e-12)
        ts = x[t]
        gt, eq = x > ts, x == ts                  # IEEE: NaN counts for nothing, -0.0 == +0.0
    eq[t] = False
    counts = []
    for lst in (None, list_a, list_b):
        keep = np.ones(n_ent, bool)
        if lst is not None:
            lst = np.asarray(lst, dtype=np.int64)
            keep[lst[(lst >= 0) & (lst < n_ent)]] = False
        keep[t] = True
        counts += [int(np.sum(gt & keep)), int(np.sum(eq & keep))]
    return logp, np.array(counts, np.int64)


def segment_eval(scores, ent, seg_ptr, target, n_ent, key_a=None, index_a=None, key_b=None, index_b=None):
    """(logp float64 [B], counts int64 [B, 6], visited bool [B]) of rg_segment_eval's inputs as numpy arrays."""
    B = len(target)
    logp, counts, visited = np.zeros(B), np.zeros((B, 6), np.int64), np.zeros(B, bool)
    for q in range(B):
        b, e = int(seg_ptr[q]), int(seg_ptr[q + 1])
        x = dense_row(scores[b:e], ent[b:e], n_ent)
        la = list_of(index_a, key_a[q]) if index_a is not None else ()
        lb = list_of(index_b, key_b[q]) if index_b is not None else ()
        logp[q], counts[q] = row_eval(x, int(target[q]), la, lb)
        visited[q] = bool(np.any(np.asarray(ent[b:e]) == target[q]))
    return logp, counts, visited


def torch_reference(x, tail):
    """The reference's sequence on a dense score matrix x [B, n_ent] (any float dtype) and tails [B]: (per-row loss terms
    log(p + 1e-12)[tail], argsort rank + 1 per row, hits@1 / @3 / @10 counts of the batch).  main.py:142,146,155-157,161-163."""
    import torch
    import torch.nn.functional as F
    score = torch.as_tensor(x)
    tail = torch.as_tensor(tail, dtype=torch.int64)
    predicted_prob = F.softmax(score, dim=1)
    logp = -F.nll_loss(torch.log(predicted_prob + 1e-12), tail, reduction="none")
    hits = [int(torch.sum(torch.topk(predicted_prob, dim=1, k=k)[1] == tail.unsqueeze(1)).item()) for k in (1, 3, 10)]
    sorted_prob = torch.argsort(predicted_prob, dim=-1, descending=True)
    ranks = torch.tensor([sorted_prob[i].eq(tail[i]).nonzero().item() for i in range(len(tail))])
    return logp.numpy(), ranks.numpy() + 1, hits


# ---- the edge case shared by tests/test_segment_eval_host.py and tests/test_segment_eval_gpu.py (built once)
N_ENT = 6000
# around the wave (64) and the workgroup (256), long ones, a single pair and the empty segment; every fourth query's target is an
# entity the segment never visited (the empty segment's among them)
LENGTHS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000, 300, 700, 64, 256, 1000, 330, 128, 513, 2, 90, 257]
ALL_NEG = (5, 12)             # the maximum comes from the implicit zeros (12: the unvisited target IS a maximum)
ALL_EQUAL = {6: -0.75, 13: 0.0}
ROUNDED = (9, 16)             # rounded to 0.1, with pairs at exactly 0.0 and -0.0 (16: an unvisited target ties with them)
SHIFT80, NEG200, WITH_NAN = 7, 10, 11
# known list length per query for the first and the second index: None = the key is absent from the index, 0 = present and empty;
# 200 / 256 at or below the kernel's LDS staging cap, 257 / 300 above it (searched in memory)
A_LEN = [5, 1, 1, 0, 200, None, 257, 300, 300, 256, 300, 40, 300, None, 2, 200, 0, 300, 257, 2, 300, 256]
B_LEN = [None, 300, 300, None, 0, 257, 200, 40, 300, 1, 256, 257, None, 300, 2, 0, 300, 257, 1, 300, 12, 200]
SHARED = (1, 2)               # these two queries share their key in both indexes
_CASE = {}


def _index_from_lists(lists):
    keys = np.array(sorted(lists), dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(lists[k]) for k in keys])]).astype(np.int64)
    idx = np.concatenate([lists[k] for k in keys] + [np.zeros(0, np.int64)]).astype(np.int32)
    return keys, ptr, idx


def edge_case():
    """dict(scores fp32 [N], ent int32 [N], seg_ptr int64 [B+1], target, key_a, index_a, key_b, index_b, where, ref=(logp, counts,
    visited)) of the 22 queries above; ``where`` is the target's position in its segment or None."""
    if _CASE:
        return _CASE
    rng = np.random.default_rng(31)
    n_q = len(LENGTHS)
    assert n_q == len(A_LEN) == len(B_LEN) == 22 and LENGTHS[0] == 0
    ents, scores, target, where = [], [], np.zeros(n_q, np.int64), {}
    for q, k in enumerate(LENGTHS):
        e = np.sort(rng.choice(N_ENT, k, replace=False))
        if q % 2:
            rng.shuffle(e)                                      # the kernel must not rely on the frontier's order
        v = (rng.standard_normal(k) * 2).astype(np.float32)     # mixed in sign: the zeros fall mid-ranking
        if q in ALL_NEG:
            v = -np.abs(v) - np.float32(0.01)
        if q in ROUNDED:
            v = np.round(v, 1)
            v[::7], v[3::7] = 0.0, -0.0
        if q in ALL_EQUAL:
            v[:] = ALL_EQUAL[q]
        if q == SHIFT80:
            v += np.float32(80)
        if q == NEG200:
            v -= np.float32(200)
        if q % 4 == 0:
            target[q] = int(np.setdiff1d(np.arange(N_ENT), e)[rng.integers(0, N_ENT - k)])
            where[q] = None
        else:
            where[q] = (0, k - 1, k // 2)[q % 3]                # first, last, middle pair
            target[q] = e[where[q]]
        if q == WITH_NAN:
            v[(where[q] + k // 3) % k] = np.nan                 # away from the target
        ents.append(e); scores.append(v)
    assert {LENGTHS[q] for q in where if where[q] is not None} >= {1, 2, 63, 65, 255, 256, 257, 1000, 5000}
    assert {0, 1, 2} <= {q % 3 for q in where if where[q] is not None} and where[0] is None
    key_a = np.array([1000 + q for q in range(n_q)], np.int64)
    key_b = np.array([5000 + 3 * q for q in range(n_q)], np.int64)
    key_a[SHARED[1]], key_b[SHARED[1]] = key_a[SHARED[0]], key_b[SHARED[0]]

    def lists_for(lens, keys, flip):
        out = {}
        for q in range(n_q):
            if lens[q] is None or int(keys[q]) in out:
                continue
            k, e = lens[q], ents[q]
            # entities of the segment (the better-scored ones first, so that the filter changes the rank), the target in every
            # other list, then entities the segment never visited; two ids outside 0..n_ent-1 in every third list
            take = e[np.argsort(-np.nan_to_num(scores[q]), kind="stable")][:k * 2 // 3] if len(e) else e
            pool = np.concatenate([[target[q]] if (q + flip) % 2 == 0 else [], [-3, N_ENT + 5] if q % 3 == 0 and k >= 3 else [], take,
                                   np.setdiff1d(np.arange(N_ENT), e)[q::7][:k + 1]]).astype(np.int64)
            _, first = np.unique(pool, return_index=True)
            out[int(keys[q])] = np.sort(pool[np.sort(first)][:k])
            assert len(out[int(keys[q])]) == k
        return out

    lists_a, lists_b = lists_for(A_LEN, key_a, 0), lists_for(B_LEN, key_b, 1)
    for lists, lens in ((lists_a, A_LEN), (lists_b, B_LEN)):    # both sides of the staging cap and the cap itself, in either index
        assert {0, 1, 200, 256, 257, 300} <= {len(v) for v in lists.values()} and None in lens
    assert any(-3 in v for v in lists_a.values()) and any(N_ENT + 5 in v for v in lists_b.values())
    index_a, index_b = _index_from_lists(lists_a), _index_from_lists(lists_b)
    seg_ptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    sc = np.concatenate(scores).astype(np.float32)
    en = np.concatenate(ents).astype(np.int32)
    ref = segment_eval(sc, en, seg_ptr, target, N_ENT, key_a, index_a, key_b, index_b)
    counts = ref[1]
    assert np.any(counts[:, 2] < counts[:, 0]) and np.any(counts[:, 4] < counts[:, 0]) and np.any(counts[:, 2] != counts[:, 4])   # the filters bite
    assert np.any(counts[:, 3] < counts[:, 1]) and np.any(counts[:, 5] < counts[:, 1])           # ... on the zeros too
    assert np.isnan(ref[0][WITH_NAN]) and np.isnan(ref[0]).sum() == 1
    _CASE.update(scores=sc, ent=en, seg_ptr=seg_ptr, target=target, key_a=key_a, index_a=index_a, key_b=key_b, index_b=index_b,
                 where=where, ref=ref)
    return _CASE
