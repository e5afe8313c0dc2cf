"""Host references of engine.trule_apply (rg_trule_apply) in numpy: what weighted temporal rules (head, body (r_1, d_1)..(r_L, d_L),
weight) predict for queries (sub[b], rel[b], ?, time[b]) on a graph given as its rows (head, rel, tail, time id) - inverse and identity
rows as the quadruples hold them, as tests/trule_ground_ref.py.  TEST INFRASTRUCTURE.

A step (r, d) admits a row (u, r, v, tau) for a query of time t iff d == 3 or tests/temporal_ref.py: direction(tau, t) == d.  Rule i
fires for cell (b, y) iff head[i] == rel[b] and its steps lead from sub[b] to y through rows each step admits for time[b].  Per cell
the rules that fire are folded in ascending i exactly as tests/rule_apply_ref.py folds them (its miss_of, initial and scores are used
here, not restated):

    fired += 1;  surv = fl32(surv * miss[i]);  if weight[i] > best: best = weight[i]; best_rule = rule_base + i

    apply_dense(...)   the definition, literally: one dense boolean matrix per (relation, time id); per rule, hop and query time t
                       the OR of the matrices of the time ids the step admits for t, then X <- (X.astype(np.int64) @ M) > 0 on the rows
                       of the queries of time t, from the subjects' rows of the unit matrix; float32 arithmetic on [B, n_ent] arrays
    apply_cells(...)   the same sets by expanding edge lists on bitmaps packed 64 columns a word (the columns of a rule: the queries
                       of its head relation sorted by time, so that the queries a row (u, v, tau) may move are one mask per (tau, d)),
                       and the fold over the firing cells only, kept in a dict b * n_ent + y -> (best, surv, best_rule, fired) as
                       rule_apply_ref.apply_cells keeps it (its cells_arrays and cells_to_dense apply).  For the larger cases.

Both take ``state`` (the four arrays / the dict of an earlier call) and ``rule_base`` (the index of rule 0 in the whole list), so a list
of rules can be applied range by range.
"""
import numpy as np

from tests.rule_apply_ref import initial, miss_of, scores  # noqa: F401  (scores: for the callers)
from tests.trule_ground_ref import ANY, FUTURE, NOW, PAST, _allowed


def _queries(subs, rels, times):
    subs, rels, times = (np.asarray(a, np.int64).reshape(-1) for a in (subs, rels, times))
    assert len(subs) == len(rels) == len(times)
    return subs, rels, times


def firing_dense(n_ent, n_rela, n_time, rows):
    """fire(h, b, dd, subs, rels, times) -> bool [B, n_ent]: the cells the rule (h, (b, dd)) fires for, by dense products."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    A = np.zeros((n_rela, n_time, n_ent, n_ent), dtype=bool)
    A[rows[:, 1], rows[:, 3], rows[:, 0], rows[:, 2]] = True

    def fire(h, b, dd, subs, rels, times):
        out = np.zeros((len(subs), n_ent), dtype=bool)
        for t in np.unique(times[rels == h]).tolist():
            q = np.nonzero((rels == h) & (times == t))[0]
            X = np.zeros((len(q), n_ent), dtype=bool)
            X[np.arange(len(q)), subs[q]] = True
            for r, d in zip(b, dd):
                M = A[r, _allowed(n_time, t, d)].any(0)
                X = (X.astype(np.int64) @ M) > 0
            out[q] = X
        return out
    return fire


def apply_dense(n_ent, n_rela, n_time, rows, head, body, direc, weight, subs, rels, times, state=None, rule_base=0):
    fire_of = firing_dense(n_ent, n_rela, n_time, rows)
    subs, rels, times = _queries(subs, rels, times)
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    best, surv, best_rule, fired = (a.copy() for a in (initial(len(subs), n_ent) if state is None else state))
    for i, (h, b, dd) in enumerate(zip(np.asarray(head).tolist(), np.asarray(body).tolist(), np.asarray(direc).tolist())):
        fire = fire_of(h, b, dd, subs, rels, times)
        fired[fire] += 1
        surv[fire] = (surv[fire] * miss[i]).astype(np.float32)
        better = fire & (weight[i] > best)
        best[better] = weight[i]
        best_rule[better] = rule_base + i
    return best, surv, best_rule, fired


def firing_packed(n_ent, n_rela, n_time, rows, subs, rels, times):
    """fire(h, b, dd) -> (b_idx, y_idx) int64 arrays of the cells the rule (h, (b, dd)) fires for among the given queries, sorted by
    (b, y): edge lists expanded on packed bitmaps, the layout of a head relation (its queries sorted by time, the masks, the seed)
    formed once."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    rows = rows[np.lexsort((rows[:, 2], rows[:, 1]))]                 # by relation, then tail
    rel_ptr = np.searchsorted(rows[:, 1], np.arange(n_rela + 1))
    layouts = {}

    def pack(m):                                                      # bool [n, bits] -> uint64 [n, bits / 64]
        return np.ascontiguousarray(np.packbits(m, axis=1)).view(np.uint64)

    def layout(h):
        q = np.nonzero(rels == h)[0]
        q = q[np.argsort(times[q], kind="stable")]
        S = len(q)
        bits = max((S + 63) // 64 * 64, 64)
        ptr = np.searchsorted(times[q], np.arange(n_time + 1))        # the first sorted query whose time is >= tau
        col = np.arange(bits)
        zero, full = np.zeros(n_time, np.int64), np.full(n_time, S)
        lo = {PAST: ptr[1:], NOW: ptr[:-1], FUTURE: zero, ANY: zero}
        hi = {PAST: full, NOW: ptr[1:], FUTURE: ptr[:-1], ANY: full}
        masks = {d: pack((col[None, :] >= lo[d][:, None]) & (col[None, :] < hi[d][:, None])) for d in (PAST, NOW, FUTURE, ANY)}
        ents = np.unique(subs[q])                                     # the seed, kept sparse: rows of the entities that are subjects
        seed = np.zeros((len(ents), bits), dtype=bool)
        seed[np.searchsorted(ents, subs[q]), np.arange(S)] = True
        return q, masks, ents, pack(seed)

    def hop(ents, X, r, d, masks):                                    # (sorted entity ids, their packed rows) -> the same of the next set
        e = rows[rel_ptr[r]:rel_ptr[r + 1]]
        at = np.searchsorted(ents, e[:, 0])
        ok = (at < len(ents)) & (ents[np.minimum(at, max(len(ents) - 1, 0))] == e[:, 0]) if len(ents) else np.zeros(len(e), bool)
        e, at = e[ok], at[ok]
        if len(e) == 0:
            return np.zeros(0, np.int64), X[:0]
        tails, starts = np.unique(e[:, 2], return_index=True)         # e is sorted by tail inside a relation
        out = np.bitwise_or.reduceat(X[at] & masks[d][e[:, 3]], starts, axis=0)
        keep = out.any(1)
        return tails[keep], out[keep]

    def fire(h, b, dd):
        if h not in layouts:
            layouts[h] = layout(h)
        q, masks, ents, X = layouts[h]
        if len(q) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        for r, d in zip(b, dd):
            ents, X = hop(ents, X, r, d, masks)
        if len(ents) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        y_at, col = np.nonzero(np.unpackbits(X.view(np.uint8), axis=1))
        bi, yi = q[col], ents[y_at]
        order = np.lexsort((yi, bi))
        return bi[order], yi[order]
    return fire


def apply_cells(n_ent, n_rela, n_time, rows, head, body, direc, weight, subs, rels, times, state=None, rule_base=0):
    subs, rels, times = _queries(subs, rels, times)
    fire = firing_packed(n_ent, n_rela, n_time, rows, subs, rels, times)
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    cells = {} if state is None else dict(state)         # b * n_ent + y -> (best, surv, best_rule, fired)
    for i, (h, b, dd) in enumerate(zip(np.asarray(head).tolist(), np.asarray(body).tolist(), np.asarray(direc).tolist())):
        bi, yi = fire(h, b, dd)
        for key in (bi * n_ent + yi).tolist():
            best, surv, rule, n = cells.get(key, (np.float32(0.0), np.float32(1.0), -1, 0))
            surv = np.float32(surv * miss[i])
            if weight[i] > best:
                best, rule = weight[i], rule_base + i
            cells[key] = (best, surv, rule, n + 1)
    return cells


# ---- typed-in cells on the hand graph of tests/trule_ground_ref.py (hand_quads(): 5 entities, 3 time ids, relations r0 r1 r2, their
# inverses 3..5 and the identity 6 at time 2).  Rows by relation as (u, v, tau):
#   r0 {(0,1,0), (0,1,2), (3,1,1), (2,4,0)}   r1 {(1,2,1), (0,2,1)}   r0^-1 {(1,0,0), (1,0,2), (1,3,1), (4,2,0)}   id {(e,e,2)}
HAND_HEAD = np.array([0, 1, 1, 1])
HAND_BODY = np.array([[0, 6],     # r0[past] ^ id -> r0 (trule_ground_ref rule 1): (0, t=1) -> 1 by (0,1,0); (0, t=2) -> 1; (2, t=1) -> 4
                      [0, 1],     # r0[any] ^ r1[now] -> r1 (rule 0): r1 has rows at time 1 only, so only queries of time 1 fire
                      [3, 0],     # r0^-1[future] ^ r0[any] -> r1 (rule 3)
                      [6, 1]])    # id ^ r1[now] -> r1: the r1 rows of the subject at the query's time
HAND_DIR = np.array([[0, 3], [3, 1], [2, 3], [3, 1]])
HAND_WEIGHT = np.array([0.5, 0.25, 0.75, 0.5], np.float32)          # miss 0.5, 0.75, 0.25, 0.5
HAND_SUBS = np.array([0, 3, 0, 1, 1, 1, 0, 0, 2])
HAND_RELS = np.array([1, 1, 1, 1, 1, 1, 0, 0, 2])
HAND_TIMES = np.array([1, 1, 0, 0, 1, 2, 2, 0, 1])
# the cells some rule reaches: (row, entity, best, surv, best_rule, fired); every other cell is (0, 1, -1, 0)
HAND_CELLS = [
    # row 0 (0, r1, t=1): rule 1: 0 -r0-> 1 (any time), 1 -r1-> 2 at time 1 = now.  rule 3: 0 -id-> 0, 0 -r1-> 2 at time 1.  Both reach
    # entity 2: fired 2, surv 0.75 * 0.5, and the later, larger weight 0.5 of rule 3 displaces rule 1's 0.25.  rule 2: 0 has no r0^-1 row
    (0, 2, 0.5, 0.375, 3, 2),
    # row 1 (3, r1, 1): rule 1: 3 -r0-> 1 (time 1), 1 -r1-> 2 now.  rule 3: 3 has no r1 row
    (1, 2, 0.25, 0.75, 1, 1),
    # row 2 (0, r1, 0): no r1 row has time 0: rules 1 and 3 reach nothing; rule 2 needs an r0^-1 row from 0: none.  No cell
    # row 3 (1, r1, 0): rule 2: r0^-1 rows from 1 later than 0: (1,0,2), (1,3,1) -> {0, 3}; r0 at any time: 0 -> 1, 3 -> 1.  Entity 1.
    #   rule 3: 1 -id-> 1, then r1 from 1 now (time 0): (1,2,1) is at time 1: nothing.  rule 1: 1 has no r0 row
    (3, 1, 0.75, 0.25, 2, 1),
    # row 4 (1, r1, 1): rule 2: later than 1: (1,0,2) -> 0 -> 1.  rule 3: 1 -id-> 1 -r1-> 2 at time 1 = now: entity 2
    (4, 1, 0.75, 0.25, 2, 1),
    (4, 2, 0.5, 0.5, 3, 1),
    # row 5 (1, r1, 2): nothing is later than the last time id, and no r1 row has time 2: no cell
    # row 6 (0, r0, t=2): rule 0: r0 rows from 0 before time 2: (0,1,0) -> 1; 1 -id-> 1
    (6, 1, 0.5, 0.5, 0, 1),
    # row 7 (0, r0, 0): nothing is before time 0: no cell.  row 8 (2, r2, 1): no rule has head r2
]


def hand_expected():
    from tests.trule_ground_ref import HAND_N_ENT
    out = initial(len(HAND_SUBS), HAND_N_ENT)
    for b, y, best, surv, rule, fired in HAND_CELLS:
        out[0][b, y], out[1][b, y], out[2][b, y], out[3][b, y] = best, surv, rule, fired
    return out
