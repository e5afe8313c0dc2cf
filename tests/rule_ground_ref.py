"""Host references of engine.rule_ground (rg_rule_ground) in numpy: the four counts of a rule (head h, body r_1..r_L) over the pairs
(x, y) with x in a source set, on a graph given as its rows (head, rel, tail) - inverse and identity rows included, a repeated row
counting once.

    rows_from_export(out_ptr, out_rel_tail)     the rows of a device graph, from Graph.export()
    rows_from_triples(n_ent, n_rel, triples)    the rows of raw base triples: inverses (t, r + n_rel, h) and the identity rows
                                                (e, 2 * n_rel, e) added here
    counts_dense(...)                           the definition, literally: one dense boolean matrix A_r per relation and the chain
                                                X <- (X.astype(np.int64) @ A_r) > 0 from the sources' rows of the unit matrix
    counts(...)                                 the same sets by expanding edge lists: next[v] |= X[u] over the edges (u, v) of r, the
                                                sources packed 64 a word.  An n_ent^3 integer product takes 40 ms at 300 entities and
                                                most of a minute at 3000, so the larger fixtures use this one;
                                                tests/test_rule_ground_ref.py holds the two equal on graphs where both are cheap.

    counts_sparse(...)                          the chain with scipy.sparse products, every entity a source: for many entities
                                                and few facts

All return int64 [R, 4] = (body_pairs, hits, pca_body_pairs, head_pairs).
"""
import numpy as np


def rows_from_export(out_ptr, out_rel_tail):
    out_ptr, rt = np.asarray(out_ptr, np.int64), np.asarray(out_rel_tail, np.int64)
    heads = np.repeat(np.arange(len(out_ptr) - 1, dtype=np.int64), np.diff(out_ptr))
    return np.stack([heads, rt[:, 0], rt[:, 1]], 1)


def rows_from_triples(n_ent, n_rel, triples):
    t = np.asarray(triples, np.int64).reshape(-1, 3)
    e = np.arange(n_ent, dtype=np.int64)
    return np.concatenate([t, np.stack([t[:, 2], t[:, 1] + n_rel, t[:, 0]], 1), np.stack([e, np.full(n_ent, 2 * n_rel), e], 1)], 0)


def _sources(n_ent, sources):
    s = np.arange(n_ent, dtype=np.int64) if sources is None else np.asarray(sources, np.int64).reshape(-1)
    assert len(np.unique(s)) == len(s) and (len(s) == 0 or (s.min() >= 0 and s.max() < n_ent))
    return s


def dense_relations(n_ent, n_rela, rows):
    """A bool [n_rela, n_ent, n_ent]: A[r, x, y] iff the graph has a row (x, r, y)."""
    rows = np.asarray(rows, np.int64)
    A = np.zeros((n_rela, n_ent, n_ent), dtype=bool)
    A[rows[:, 1], rows[:, 0], rows[:, 2]] = True
    return A


def _four(X, H):
    """The counts from body and head reachability bool [S, n_ent]."""
    has_head = H.any(1)
    return [int(X.sum()), int((X & H).sum()), int(X[has_head].sum()), int(H.sum())]


def counts_dense(n_ent, n_rela, rows, head, body, sources=None):
    A = dense_relations(n_ent, n_rela, rows)
    s = _sources(n_ent, sources)
    seed = np.zeros((len(s), n_ent), dtype=bool)
    seed[np.arange(len(s)), s] = True
    out = []
    for h, b in zip(np.asarray(head).tolist(), np.asarray(body).tolist()):
        X = seed
        for r in b:
            X = (X.astype(np.int64) @ A[r]) > 0
        H = (seed.astype(np.int64) @ A[h]) > 0
        out.append(_four(X, H))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def _popcount(m):
    """Number of set bits of a uint64 array."""
    if hasattr(np, "bitwise_count"):
        return int(np.bitwise_count(m).sum(dtype=np.int64))
    return int(np.unpackbits(m.view(np.uint8)).sum(dtype=np.int64))


def counts(n_ent, n_rela, rows, head, body, sources=None):
    rows = np.asarray(rows, np.int64)
    s = _sources(n_ent, sources)
    by_rel = {}
    for r in range(n_rela):                              # the edges of r ordered by tail, and where each tail's run starts
        e = rows[rows[:, 1] == r]
        e = e[np.argsort(e[:, 2], kind="stable")]
        tails, starts = np.unique(e[:, 2], return_index=True)
        by_rel[r] = (e[:, 0], tails, starts)

    def hop(X, r):                                       # X uint64 [n_ent, ceil(S / 64)]: entity-major, the sources packed 64 a word
        us, tails, starts = by_rel[r]
        out = np.zeros_like(X)
        if len(us):
            out[tails] = np.bitwise_or.reduceat(X[us], starts, axis=0)
        return out

    def four(X, H):
        has_head = np.bitwise_or.reduce(H, axis=0)
        return [_popcount(m) for m in (X, X & H, X & has_head, H)]

    seed = np.zeros((n_ent, (len(s) + 63) // 64 * 64), dtype=bool)
    seed[s, np.arange(len(s))] = True
    seed = np.ascontiguousarray(np.packbits(seed, axis=1)).view(np.uint64)
    heads, stack, out = {}, [((), seed)], []             # stack[l]: the reach of the body prefix of length l last formed
    for h, b in zip(np.asarray(head).tolist(), np.asarray(body).tolist()):
        keep = 1
        while keep < len(stack) and keep <= len(b) and stack[keep][0] == tuple(b[:keep]):
            keep += 1
        del stack[keep:]
        for l in range(keep, len(b) + 1):
            stack.append((tuple(b[:l]), hop(stack[-1][1], b[l - 1])))
        if h not in heads:
            heads[h] = hop(seed, h)
        out.append(four(stack[-1][1], heads[h]))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def counts_sparse(n_ent, n_rela, rows, head, body):
    """The product chain once more with scipy.sparse matrices, every entity a source: for a graph of many entities and few facts,
    where the bitmaps of ``counts`` would hold gigabytes of zeros."""
    import scipy.sparse as sp
    rows = np.asarray(rows, np.int64)
    A = []
    for r in range(n_rela):
        e = np.unique(rows[rows[:, 1] == r], axis=0)
        A.append(sp.csr_matrix((np.ones(len(e), np.int64), (e[:, 0], e[:, 2])), shape=(n_ent, n_ent)))
    out = []
    for h, b in zip(np.asarray(head).tolist(), np.asarray(body).tolist()):
        X = A[b[0]]
        for r in b[1:]:
            X = (X @ A[r]).tocsr()
            X.data[:] = 1                                # path counts are positive: every stored entry is a pair
        has_head = np.diff(A[h].indptr) > 0
        out.append([X.nnz, X.multiply(A[h]).nnz, int(np.diff(X.indptr)[has_head].sum()), A[h].nnz])
    return np.array(out, dtype=np.int64).reshape(-1, 4)


# ---- a graph small enough to count by hand --------------------------------------------------------------------------
# 5 entities, 2 relations: ids 0 = r0, 1 = r1, 2 = r0^-1, 3 = r1^-1, 4 = identity.  (0, r0, 1) is stated twice.
HAND_N_ENT, HAND_N_REL = 5, 2
HAND_TRIPLES = np.array([[0, 0, 1], [0, 0, 1], [1, 1, 2], [0, 1, 2], [3, 0, 1], [3, 1, 4], [2, 0, 4]])
# A_0 = {01, 31, 24}, A_1 = {12, 02, 34}, A_2 = {10, 13, 42}, A_3 = {21, 20, 43}
HAND_HEAD = np.array([1, 0, 0, 1, 0])
HAND_BODY = np.array([[0, 1],     # r0 ^ r1 -> r1: body {02, 32}, of which 02 is an r1 fact; 0 and 3 both have r1 facts
                      [1, 2],     # r1 ^ r0^-1 -> r0 (an inverse step): body {32}, no r0 fact; 3 has one
                      [4, 0],     # id ^ r0 -> r0 (an identity step; the trivial rule): body = A_0, the duplicate counted once
                      [0, 0],     # r0 ^ r0 -> r1: no grounding
                      [1, 3]])    # r1 ^ r1^-1 -> r0: body {11, 10, 01, 00, 33}, 01 an r0 fact; 1 has no r0 fact
HAND_ALL = np.array([[2, 1, 2, 3], [1, 0, 1, 3], [3, 3, 3, 3], [0, 0, 0, 3], [5, 1, 3, 3]])
HAND_SOURCES = np.array([3, 0])
HAND_SUB = np.array([[2, 1, 2, 2], [1, 0, 1, 2], [2, 2, 2, 2], [0, 0, 0, 2], [3, 1, 3, 2]])


def hand_rows():
    return rows_from_triples(HAND_N_ENT, HAND_N_REL, HAND_TRIPLES)


# ---- many entities, few facts: the shape that takes the bitmaps of a call past 2^31 words at little cost -----------------------
def wide_graph(n_ent, seed=9):
    """(n_ent, n_rel, number of relation ids, base triples): 160 facts of relations 0 and 1 (9 of them twice) among the first 20
    and the last 20 entities; relation 2 has no fact."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([np.arange(20), np.arange(n_ent - 20, n_ent)])
    trip = np.stack([pool[rng.integers(0, 40, 160)], rng.integers(0, 2, 160), pool[rng.integers(0, 40, 160)]], 1)
    return n_ent, 3, 7, np.concatenate([trip, trip[:9]], 0)


def wide_rules(n_rela, n=17, seed=10):
    """n rules of length 2 over all relation ids (identity, inverses and the empty relation among them); the last two are
    id ^ id -> id, which every entity grounds, and r0 ^ r1 -> r1."""
    rng = np.random.default_rng(seed)
    head, body = rng.integers(0, n_rela, n), rng.integers(0, n_rela, (n, 2))
    head[-2], body[-2] = n_rela - 1, (n_rela - 1, n_rela - 1)
    head[-1], body[-1] = 1, (0, 1)
    return head, body
