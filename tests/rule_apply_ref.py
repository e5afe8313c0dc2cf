"""Host references of engine.rule_apply (rg_rule_apply) in numpy: what weighted rules (head, body r_1..r_L, weight) predict for queries
(sub[b], rel[b], ?) on a graph given as its rows (head, rel, tail) - inverse and identity rows included, as tests/rule_ground_ref.py.
TEST INFRASTRUCTURE.

Rule i fires for cell (b, y) iff head[i] == rel[b] and body_i(sub[b], y).  Per cell, from best = 0, surv = 1, best_rule = -1, fired = 0,
the rules that fire are visited in ascending i:

    fired += 1;  surv = fl32(surv * miss[i]);  if weight[i] > best: best = weight[i]; best_rule = i        miss[i] = fl32(1 - weight[i])

    apply_dense(...)     the definition, literally: one dense boolean matrix A_r per relation, a Python loop over the rules in order
                         with the chain X <- (X.astype(np.int64) @ A_r) > 0 from the subjects' rows of the unit matrix, float32
                         arithmetic on [B, n_ent] arrays
    apply_cells(...)     the same with scipy.sparse products and the fold over the firing cells only, kept in a dict: for a graph of
                         many entities and few facts, where dense arrays would hold gigabytes of defaults.  Returns the cells that some
                         rule reaches: (b, y, best, surv, best_rule, fired) arrays sorted by (b, y)
    cells_to_dense(...)  those cells scattered into the default arrays
    scores(...)          "max" = best, "noisy_or" = fl32(1 - surv)

Both take ``state`` (the four arrays / the dict of an earlier call) and ``rule_base`` (the index of rule 0 in the whole list), so a list
of rules can be applied range by range.
"""
import numpy as np

from tests import rule_ground_ref as G


def miss_of(weight):
    return (np.float32(1.0) - np.asarray(weight, np.float32)).astype(np.float32)


def initial(B, n_ent):
    return (np.zeros((B, n_ent), np.float32), np.ones((B, n_ent), np.float32), np.full((B, n_ent), -1, np.int32),
            np.zeros((B, n_ent), np.int32))


def apply_dense(n_ent, n_rela, rows, head, body, weight, subs, rels, state=None, rule_base=0):
    A = G.dense_relations(n_ent, n_rela, rows)
    subs, rels = np.asarray(subs, np.int64).reshape(-1), np.asarray(rels, np.int64).reshape(-1)
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    best, surv, best_rule, fired = (a.copy() for a in (initial(len(subs), n_ent) if state is None else state))
    for i, (h, b) in enumerate(zip(np.asarray(head).tolist(), np.asarray(body).tolist())):
        q = np.nonzero(rels == h)[0]
        X = np.zeros((len(q), n_ent), dtype=bool)
        X[np.arange(len(q)), subs[q]] = True
        for r in b:
            X = (X.astype(np.int64) @ A[r]) > 0
        fire = np.zeros((len(subs), n_ent), dtype=bool)
        fire[q] = X
        fired[fire] += 1
        surv[fire] = (surv[fire] * miss[i]).astype(np.float32)
        better = fire & (weight[i] > best)
        best[better] = weight[i]
        best_rule[better] = rule_base + i
    return best, surv, best_rule, fired


def firing_sparse(n_ent, n_rela, rows):
    """fire(h, b, subs, rels) -> (b_idx, y_idx) int64 arrays of the cells a rule (h, b) fires for, by scipy.sparse products."""
    import scipy.sparse as sp
    rows = np.asarray(rows, np.int64)
    A = []
    for r in range(n_rela):
        e = np.unique(rows[rows[:, 1] == r], axis=0)
        A.append(sp.csr_matrix((np.ones(len(e), np.int64), (e[:, 0], e[:, 2])), shape=(n_ent, n_ent)))

    def fire(h, b, subs, rels):
        q = np.nonzero(rels == h)[0]
        X = sp.csr_matrix((np.ones(len(q), np.int64), (np.arange(len(q)), subs[q])), shape=(len(q), n_ent))
        for r in b:
            X = (X @ A[r]).tocsr()
            X.data[:] = 1                                # path counts are positive: every stored entry is a pair
        X = X.tocoo()
        return q[X.row], X.col.astype(np.int64)
    return fire


def apply_cells(n_ent, n_rela, rows, head, body, weight, subs, rels, state=None, rule_base=0):
    fire = firing_sparse(n_ent, n_rela, rows)
    subs, rels = np.asarray(subs, np.int64).reshape(-1), np.asarray(rels, np.int64).reshape(-1)
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    cells = {} if state is None else dict(state)         # b * n_ent + y -> (best, surv, best_rule, fired)
    for i, (h, b) in enumerate(zip(np.asarray(head).tolist(), np.asarray(body).tolist())):
        bi, yi = fire(h, b, subs, rels)
        for key in (bi * n_ent + yi).tolist():
            best, surv, rule, n = cells.get(key, (np.float32(0.0), np.float32(1.0), -1, 0))
            surv = np.float32(surv * miss[i])
            if weight[i] > best:
                best, rule = weight[i], rule_base + i
            cells[key] = (best, surv, rule, n + 1)
    return cells


def cells_arrays(cells, n_ent):
    """(b, y int64, best, surv float32, best_rule, fired int32) of a dict of apply_cells, sorted by (b, y)."""
    keys = np.array(sorted(cells), dtype=np.int64)
    col = lambda c, dt: np.array([cells[k][c] for k in keys.tolist()], dtype=dt)
    return keys // n_ent, keys % n_ent, col(0, np.float32), col(1, np.float32), col(2, np.int32), col(3, np.int32)


def cells_to_dense(cells, B, n_ent):
    b, y, best, surv, rule, fired = cells_arrays(cells, n_ent)
    out = initial(B, n_ent)
    for a, v in zip(out, (best, surv, rule, fired)):
        a[b, y] = v
    return out


def scores(best, surv, agg):
    assert agg in ("max", "noisy_or")
    return np.asarray(best, np.float32) if agg == "max" else (np.float32(1.0) - np.asarray(surv, np.float32)).astype(np.float32)


def order(score, drop=()):
    """Entity ids of one score row, score descending then id ascending, without the ids in ``drop``."""
    keep = np.setdiff1d(np.arange(len(score)), np.asarray(drop, np.int64))
    return keep[np.lexsort((keep, -score[keep].astype(np.float64)))]


# ---- the hand graph of tests/rule_ground_ref.py (A_0 = {01, 31, 24}, A_1 = {12, 02, 34}, A_2 = {10, 13, 42}, A_3 = {21, 20, 43}, 4 = id)
HAND_HEAD = np.array([0, 0, 0, 0, 1, 1])
HAND_BODY = np.array([[1, 2],     # r1 ^ r0^-1 -> r0: body {32}
                      [1, 3],     # r1 ^ r1^-1 -> r0: body {11, 10, 01, 00, 33}
                      [4, 0],     # id ^ r0 -> r0 (trivial): body A_0 = {01, 31, 24}
                      [4, 4],     # id ^ id -> r0: body {00, 11, 22, 33, 44}
                      [0, 0],     # r0 ^ r0 -> r1: no grounding
                      [0, 1]])    # r0 ^ r1 -> r1: body {02, 32}
HAND_WEIGHT = np.array([0.5, 0.75, 0.75, 1.0, 0.9, 0.125], np.float32)         # miss 0.5, 0.25, 0.25, 0, fl32(1 - fl32(0.9)), 0.875
HAND_SUBS = np.array([0, 3, 0, 3, 0, 1, 2])
HAND_RELS = np.array([1, 0, 0, 1, 0, 0, 3])              # row 4 repeats row 2; relation 3 has a query and no rule
# the cells some rule reaches: (row, entity, best, surv, best_rule, fired); every other cell is (0, 1, -1, 0)
HAND_CELLS = [
    (0, 2, 0.125, 0.875, 5, 1),    # (0, r1): r0 ^ r1 reaches exactly entity 2
    (1, 1, 0.75, 0.25, 2, 1),      # (3, r0): 31 by rule 2
    (1, 2, 0.5, 0.5, 0, 1),        #          32 by rule 0
    (1, 3, 1.0, 0.0, 3, 2),        #          33 by rules 1 and 3: the later, larger weight wins; 0.25 * 0 = 0
    (2, 0, 1.0, 0.0, 3, 2),        # (0, r0): 00 by rules 1 and 3
    (2, 1, 0.75, 0.0625, 1, 2),    #          01 by rules 1 and 2 of equal weight: the first wins; 0.25 * 0.25
    (3, 2, 0.125, 0.875, 5, 1),    # (3, r1): 32 by rule 5
    (4, 0, 1.0, 0.0, 3, 2),        # row 2 again
    (4, 1, 0.75, 0.0625, 1, 2),
    (5, 0, 0.75, 0.25, 1, 1),      # (1, r0): 10 by rule 1
    (5, 1, 1.0, 0.0, 3, 2),        #          11 by rules 1 and 3
]


def hand_expected():
    out = initial(len(HAND_SUBS), G.HAND_N_ENT)
    for b, y, best, surv, rule, fired in HAND_CELLS:
        out[0][b, y], out[1][b, y], out[2][b, y], out[3][b, y] = best, surv, rule, fired
    return out


def same(a, b):
    """Four arrays equal bit for bit (float32 compared as their bit patterns) and in dtype."""
    return all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))
