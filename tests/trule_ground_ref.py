"""Host references of engine.trule_ground (rg_trule_ground) in numpy: the four counts of a temporal rule (head h, body (r_1, d_1) ..
(r_L, d_L)) over the pairs ((x, t), y) with (x, t) in an anchor set, on a graph given as its rows (head, rel, tail, time id) - inverse
and identity rows as the quadruples hold them, a repeated row counting once.  d is tests/temporal_ref.py: direction() of the edge's
time against the anchor's (0 past, 1 now, 2 future); 3 = any.  The head is a "now" step: head(x, y | t) iff the row (x, h, y, t) exists.

    default_anchors(rows, n_ent, n_rela)   the distinct (head, time) of the non-identity rows, sorted by (time, entity)
    counts_dense(...)                      the definition, literally: one dense boolean matrix per (relation, time id); per hop and
                                           anchor time t the OR of the matrices of the time ids the direction allows for t, then
                                           X <- (X.astype(np.int64) @ M) > 0 on the rows of the anchors of time t
    counts(...)                            the same sets by expanding edge lists: next[v] |= X[u] & columns(tau, d) over the edges
                                           (u, v, tau) of r, the anchors (sorted by time) packed 64 a word, columns(tau, d) the anchors
                                           whose time stands to tau as d says.  The dense form takes minutes beyond a few hundred
                                           anchors, so the larger cases use this one; tests/test_trule_ground_ref.py holds the two
                                           equal where both are cheap.

Both return int64 [R, 4] = (body_pairs, hits, pca_body_pairs, head_pairs), and both take the anchors in any order (counts are sums).
"""
import numpy as np

from tests.rule_ground_ref import _four, _popcount
from tests.temporal_ref import direction

PAST, NOW, FUTURE, ANY = 0, 1, 2, 3


def default_anchors(rows, n_ent, n_rela):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    rows = rows[rows[:, 1] != n_rela - 1]
    key = np.unique(rows[:, 3] * n_ent + rows[:, 0])
    return np.stack([key % n_ent, key // n_ent], 1)


def _anchors(rows, n_ent, n_rela, n_time, anchors):
    a = default_anchors(rows, n_ent, n_rela) if anchors is None else np.asarray(anchors, np.int64).reshape(-1, 2)
    assert len(np.unique(a, axis=0)) == len(a)
    assert len(a) == 0 or (a.min() >= 0 and a[:, 0].max() < n_ent and a[:, 1].max() < n_time)
    return a[np.lexsort((a[:, 0], a[:, 1]))]


def _allowed(n_time, t, d):
    """The edge time ids a step of direction d admits for an anchor of time t."""
    taus = np.arange(n_time)
    return taus if d == ANY else taus[direction(taus, t) == d]


def counts_dense(n_ent, n_rela, n_time, rows, head, body, direc, anchors=None):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    a = _anchors(rows, n_ent, n_rela, n_time, anchors)
    A = np.zeros((n_rela, n_time, n_ent, n_ent), dtype=bool)
    A[rows[:, 1], rows[:, 3], rows[:, 0], rows[:, 2]] = True
    seed = np.zeros((len(a), n_ent), dtype=bool)
    seed[np.arange(len(a)), a[:, 0]] = True
    times = np.unique(a[:, 1])

    def hop(X, r, d):
        out = np.zeros_like(X)
        for t in times.tolist():
            at = a[:, 1] == t
            M = A[r, _allowed(n_time, t, d)].any(0)
            out[at] = (X[at].astype(np.int64) @ M) > 0
        return out

    out = []
    for h, b, dd in zip(np.asarray(head).tolist(), np.asarray(body).tolist(), np.asarray(direc).tolist()):
        X = seed
        for r, d in zip(b, dd):
            X = hop(X, r, d)
        out.append(_four(X, hop(seed, h, NOW)))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def counts(n_ent, n_rela, n_time, rows, head, body, direc, anchors=None):
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    a = _anchors(rows, n_ent, n_rela, n_time, anchors)
    S = len(a)
    bits = max((S + 63) // 64 * 64, 64)
    ptr = np.searchsorted(a[:, 1], np.arange(n_time + 1))            # the first sorted anchor whose time is >= tau

    def pack(m):                                                      # bool [n, bits] -> uint64 [n, bits / 64]
        return np.ascontiguousarray(np.packbits(m, axis=1)).view(np.uint64)

    col = np.arange(bits)
    lo = {PAST: ptr[1:], NOW: ptr[:-1], FUTURE: np.zeros(n_time, np.int64), ANY: np.zeros(n_time, np.int64)}
    hi = {PAST: np.full(n_time, S), NOW: ptr[1:], FUTURE: ptr[:-1], ANY: np.full(n_time, S)}
    masks = {d: pack((col[None, :] >= lo[d][:, None]) & (col[None, :] < hi[d][:, None])) for d in (PAST, NOW, FUTURE, ANY)}

    order = np.lexsort((rows[:, 2], rows[:, 1]))                      # by relation, then tail
    rows = rows[order]
    rel_ptr = np.searchsorted(rows[:, 1], np.arange(n_rela + 1))

    def hop(X, r, d):                                                 # X uint64 [n_ent, bits / 64]: entity-major
        e = rows[rel_ptr[r]:rel_ptr[r + 1]]
        out = np.zeros_like(X)
        if len(e):
            tails, starts = np.unique(e[:, 2], return_index=True)
            out[tails] = np.bitwise_or.reduceat(X[e[:, 0]] & masks[d][e[:, 3]], starts, axis=0)
        return out

    def four(X, H):
        has_head = np.bitwise_or.reduce(H, axis=0)
        return [_popcount(m) for m in (X, X & H, X & has_head, H)]

    seed = np.zeros((n_ent, bits), dtype=bool)
    seed[a[:, 0], np.arange(S)] = True
    seed = pack(seed)
    heads, out = {}, []
    for h, b, dd in zip(np.asarray(head).tolist(), np.asarray(body).tolist(), np.asarray(direc).tolist()):
        X = seed
        for r, d in zip(b, dd):
            X = hop(X, r, d)
        if h not in heads:
            heads[h] = hop(seed, h, NOW)
        out.append(four(X, heads[h]))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def random_rules(rng, n, n_rela, max_hops=3):
    """{L: (head [n_L], body [n_L, L], direction [n_L, L])} for L in 1..max_hops, n rules in all: relations over all ids, directions
    over 0..3, heads among the non-identity ids."""
    out = {}
    for L in range(1, max_hops + 1):
        k = n // max_hops + (1 if L <= n % max_hops else 0)
        out[L] = (rng.integers(0, n_rela - 1, k), rng.integers(0, n_rela, (k, L)), rng.integers(0, 4, (k, L)))
    return out


# ---- a graph small enough to count by hand --------------------------------------------------------------------------
# 5 entities, 3 time ids, relations 0 = r0, 1 = r1, 2 = r2 (no fact), 3..5 their inverses, 6 = identity (at time 2, the sentinel).
# (0, r0, 1) is stated at times 0 and 2; (1, r1, 2, 1) is given twice.
HAND_N_ENT, HAND_N_REL, HAND_N_RELA, HAND_N_TIME = 5, 3, 7, 3
HAND_BASE = np.array([[0, 0, 1, 0], [0, 0, 1, 2], [1, 1, 2, 1], [1, 1, 2, 1], [0, 1, 2, 1], [3, 0, 1, 1], [2, 0, 4, 0]])
# rows by relation as (u, v, tau):  r0 {(0,1,0), (0,1,2), (3,1,1), (2,4,0)}   r1 {(1,2,1), (0,2,1)}
#                                    r0^-1 {(1,0,0), (1,0,2), (1,3,1), (4,2,0)}   r1^-1 {(2,1,1), (2,0,1)}   id {(e,e,2)}
# default anchors (entity, time): time 0 {0, 1, 2, 4}, time 1 {0, 1, 2, 3}, time 2 {0, 1}: 10 in all
HAND_ANCHORS = np.array([[0, 0], [1, 0], [2, 0], [4, 0], [0, 1], [1, 1], [2, 1], [3, 1], [0, 2], [1, 2]])
HAND_HEAD = np.array([1, 0, 0, 1, 0, 2])
HAND_BODY = np.array([[0, 1],     # r0 ^ r1[now] -> r1: r1 has rows at time 1 only; ((0,1), 2) and ((3,1), 2); (0, r1, 2, 1) is a fact
                      [0, 6],     # r0[past] ^ id -> r0 (an identity step): ((0,1), 1), ((0,2), 1), ((2,1), 4); only (0, r0, 1, 2) is a fact
                      [6, 0],     # id ^ r0[now] -> r0, the trivial rule: body = head; the fact at two times counts under each
                      [3, 0],     # r0^-1[future] ^ r0 -> r1: ((1,0), 1) and ((1,1), 1); no r1 fact 1 -> 1; anchor (1,1) has an r1 fact
                      [2, 0],     # r2 ^ r0[now] -> r0: an empty relation
                      [0, 1]])    # r0[now] ^ r1[now] -> r2: ((3,1), 2); the head relation has no fact
HAND_DIR = np.array([[3, 1], [0, 3], [3, 1], [2, 3], [3, 1], [1, 1]])
HAND_ALL = np.array([[2, 1, 1, 2], [3, 1, 1, 4], [4, 4, 4, 4], [2, 0, 1, 2], [0, 0, 0, 4], [1, 0, 0, 0]])
HAND_SUBSET = np.array([[0, 2], [3, 1]])     # given out of time order
HAND_SUB = np.array([[1, 0, 0, 0], [1, 1, 1, 2], [2, 2, 2, 2], [0, 0, 0, 0], [0, 0, 0, 2], [1, 0, 0, 0]])


def hand_quads():
    """The hand graph as the quadruples a caller gives: base rows, inverses (t, r + n_rel, h, time) and the identity rows at the
    sentinel time n_time - 1.  int64 [n, 4]."""
    q = HAND_BASE
    ent = np.arange(HAND_N_ENT)
    return np.concatenate([q, np.column_stack([q[:, 2], q[:, 1] + HAND_N_REL, q[:, 0], q[:, 3]]),
                           np.column_stack([ent, np.full(HAND_N_ENT, HAND_N_RELA - 1), ent, np.full(HAND_N_ENT, HAND_N_TIME - 1)])], 0)
