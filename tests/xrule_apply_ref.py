"""Host references of engine.xrule_apply (rg_xrule_apply) in numpy: what weighted extrapolation rules (head, body (r_1, [lo_1, hi_1))
.. (r_L, [lo_L, hi_L)), weight) forecast for queries (sub[b], rel[b], ?, day[b]) on the forecasting model's data, given as
tests/xrule_ground_ref.py takes it: rows data[j] = (s, r, o, ts) sorted by time, row_day[j], and the row window [win_lo[t], win_hi[t])
of every query day.  TEST INFRASTRUCTURE.

A step (r, [lo, hi)) admits the data row j = (u, r, v) for a query of day t iff win_lo[t] <= j < win_hi[t] and lo <= t - row_day[j] <
hi; the identity relation n_rel stands for the self-loops, admitted iff lo <= min(t, loop_window) < hi - exactly what
xrule_ground_ref admits for an anchor of day t.  Rule i fires for cell (b, y) iff head[i] == rel[b] and its steps lead from sub[b] to
y through rows each step admits for day[b]; there is no head pass.  Per cell the rules that fire are folded in ascending i exactly as
tests/rule_apply_ref.py folds them (its miss_of, initial, scores and cells helpers are used here, not restated):

    fired += 1;  surv = fl32(surv * miss[i]);  if weight[i] > best: best = weight[i]; best_rule = rule_base + i

    apply_dense(...)   the definition, literally: per query day and step one dense boolean n_ent x n_ent matrix of the admitted rows,
                       as xrule_ground_ref.counts_dense forms it, then X <- (X.astype(np.int64) @ M) > 0 on the rows of the queries of
                       that day, from the subjects' rows of the unit matrix; float32 arithmetic on [B, n_ent] arrays
    apply_cells(...)   the same sets by expanding edge lists, day by day: out[v] |= X[u] over the admitted rows (u, v), entity-major
                       with the day's queries for columns, and the fold over the firing cells only, kept in a dict b * n_ent + y ->
                       (best, surv, best_rule, fired) as rule_apply_ref.apply_cells keeps it.  For the larger cases.
    apply_lists(...)   apply_cells' firing cells under apply_dense's fold on [B, n_ent] arrays: for thousands of queries over a few
                       hundred entities, where most cells fire and a dict entry per cell is the slow part

All take ``state`` (the four arrays / the dict of an earlier call) and ``rule_base`` (the index of rule 0 in the whole list), so a list
of rules can be applied range by range.
"""
import numpy as np

from tests.rule_apply_ref import cells_arrays, cells_to_dense, initial, miss_of, same, scores  # noqa: F401  (for the callers too)
from tests.xrule_ground_ref import WINDOW, _loop_ok


def _queries(subs, rels, days):
    subs, rels, days = (np.asarray(a, np.int64).reshape(-1) for a in (subs, rels, days))
    assert len(subs) == len(rels) == len(days)
    return subs, rels, days


def _rules(head, body, lag_lo, lag_hi):
    return zip(*(np.asarray(x, np.int64).tolist() for x in (head, body, lag_lo, lag_hi)))


def firing_dense(n_ent, n_rel, data, row_day, win_lo, win_hi, loop_window=WINDOW):
    """fire(h, b, los, his, subs, rels, days) -> bool [B, n_ent]: the cells the rule fires for, by dense products."""
    data, row_day = np.asarray(data, np.int64).reshape(-1, 4), np.asarray(row_day, np.int64)

    def matrix(t, r, lo, hi):
        M = np.zeros((n_ent, n_ent), dtype=bool)
        if r == n_rel:
            if _loop_ok(t, lo, hi, loop_window):
                M[np.arange(n_ent), np.arange(n_ent)] = True
            return M
        for j in range(int(win_lo[t]), int(win_hi[t])):
            if data[j, 1] == r and lo <= t - row_day[j] < hi:
                M[data[j, 0], data[j, 2]] = True
        return M

    def fire(h, b, los, his, subs, rels, days):
        out = np.zeros((len(subs), n_ent), dtype=bool)
        for t in np.unique(days[rels == h]).tolist():
            q = np.nonzero((rels == h) & (days == t))[0]
            X = np.zeros((len(q), n_ent), dtype=bool)
            X[np.arange(len(q)), subs[q]] = True
            for r, lo, hi in zip(b, los, his):
                X = (X.astype(np.int64) @ matrix(t, r, lo, hi)) > 0
            out[q] = X
        return out
    return fire


def _fold_arrays(fire_of, n_ent, rules, weight, B, state, rule_base):
    """The fold on [B, n_ent] arrays: fire_of(h, b, los, his) -> bool [B, n_ent] per rule, in order."""
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    best, surv, best_rule, fired = (a.copy() for a in (initial(B, n_ent) if state is None else state))
    for i, rule in enumerate(rules):
        fire = fire_of(*rule)
        fired[fire] += 1
        surv[fire] = (surv[fire] * miss[i]).astype(np.float32)
        better = fire & (weight[i] > best)
        best[better] = weight[i]
        best_rule[better] = rule_base + i
    return best, surv, best_rule, fired


def apply_dense(n_ent, n_rel, data, row_day, win_lo, win_hi, head, body, lag_lo, lag_hi, weight, subs, rels, days, state=None,
                rule_base=0, loop_window=WINDOW):
    fire_of = firing_dense(n_ent, n_rel, data, row_day, win_lo, win_hi, loop_window)
    subs, rels, days = _queries(subs, rels, days)
    return _fold_arrays(lambda *rule: fire_of(*rule, subs, rels, days), n_ent, _rules(head, body, lag_lo, lag_hi), weight, len(subs), state,
                        rule_base)


def firing_lists(n_ent, n_rel, data, row_day, win_lo, win_hi, subs, rels, days, loop_window=WINDOW):
    """fire(h, b, los, his) -> (b_idx, y_idx) int64 arrays of the cells the rule fires for among the given queries, sorted by (b, y):
    edge lists expanded day by day; the rows of a day's window and their lags are formed once per day."""
    data, row_day = np.asarray(data, np.int64).reshape(-1, 4), np.asarray(row_day, np.int64)
    s, rel, o = data[:, 0], data[:, 1], data[:, 2]
    window = {}

    def rows_of(t):
        if t not in window:
            idx = np.arange(int(win_lo[t]), max(int(win_hi[t]), int(win_lo[t])))
            window[t] = (idx, t - row_day[idx])
        return window[t]

    def expand(X, u, v):                                              # X bool [n_ent, S_t]: out[v] |= X[u] over the edges (u, v)
        res = np.zeros_like(X)
        if len(u):
            order = np.argsort(v, kind="stable")
            tails, starts = np.unique(v[order], return_index=True)
            res[tails] = np.logical_or.reduceat(X[u[order]], starts, axis=0)
        return res

    def fire(h, b, los, his):
        bi, yi = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
        for t in np.unique(days[rels == h]).tolist():
            q = np.nonzero((rels == h) & (days == t))[0]
            X = np.zeros((n_ent, len(q)), dtype=bool)
            X[subs[q], np.arange(len(q))] = True
            idx, lag = rows_of(t)
            for r, lo, hi in zip(b, los, his):
                if r == n_rel:
                    X = X if _loop_ok(t, lo, hi, loop_window) else np.zeros_like(X)
                else:
                    e = idx[(rel[idx] == r) & (lag >= lo) & (lag < hi)]
                    X = expand(X, s[e], o[e])
            y, col = np.nonzero(X)
            bi.append(q[col])
            yi.append(y.astype(np.int64))
        bi, yi = np.concatenate(bi), np.concatenate(yi)
        order = np.lexsort((yi, bi))
        return bi[order], yi[order]
    return fire


def apply_cells(n_ent, n_rel, data, row_day, win_lo, win_hi, head, body, lag_lo, lag_hi, weight, subs, rels, days, state=None,
                rule_base=0, loop_window=WINDOW):
    subs, rels, days = _queries(subs, rels, days)
    fire = firing_lists(n_ent, n_rel, data, row_day, win_lo, win_hi, subs, rels, days, loop_window)
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    cells = {} if state is None else dict(state)         # b * n_ent + y -> (best, surv, best_rule, fired)
    for i, (h, b, los, his) in enumerate(_rules(head, body, lag_lo, lag_hi)):
        bi, yi = fire(h, b, los, his)
        for key in (bi * n_ent + yi).tolist():
            best, surv, rule, n = cells.get(key, (np.float32(0.0), np.float32(1.0), -1, 0))
            surv = np.float32(surv * miss[i])
            if weight[i] > best:
                best, rule = weight[i], rule_base + i
            cells[key] = (best, surv, rule, n + 1)
    return cells


def apply_lists(n_ent, n_rel, data, row_day, win_lo, win_hi, head, body, lag_lo, lag_hi, weight, subs, rels, days, state=None,
                rule_base=0, loop_window=WINDOW):
    """apply_cells' firing cells under apply_dense's fold: four [B, n_ent] arrays (``state`` too), for many queries over few entities,
    where a dict entry per cell is the slow part."""
    subs, rels, days = _queries(subs, rels, days)
    fire = firing_lists(n_ent, n_rel, data, row_day, win_lo, win_hi, subs, rels, days, loop_window)

    def fire_of(*rule):
        out = np.zeros((len(subs), n_ent), dtype=bool)
        out[fire(*rule)] = True
        return out
    return _fold_arrays(fire_of, n_ent, _rules(head, body, lag_lo, lag_hi), weight, len(subs), state, rule_base)


def sort_by_head(head, *per_rule):
    """The rules stably sorted by head: (order, head[order], x[order] for every x)."""
    order = np.argsort(np.asarray(head), kind="stable")
    return (order, np.asarray(head)[order]) + tuple(np.asarray(x)[order] for x in per_rule)


# ---- the hand data set of tests/xrule_ground_ref.py with its 7 rules stably sorted by head (original order [0, 3, 6, 1, 2, 4, 5]) and
# ten queries (s, p, day), q0 .. q9.  The firing cells (query, entity) per sorted rule, typed in; nothing else fires:
#   0  id ^ r0[0-1d] -> r0               (q3, 1) by row 0 at day 1; (q4, 1) by row 8 at day 123
#   1  r2 ^ r0 -> r0                     none: r2 has no row
#   2  id[61-120d] ^ r0 -> r0            a self-loop's lag is min(t, 120) = 120 at day 123: (q4, 1) by rows 0, 2, 8; (q5, 3) by row 7
#   3  r0[121+] ^ r1 -> r1               day 123: rows 0, 2 (0 -> 1), then 1 -> 2 by rows 1, 4: (q1, 2)
#   4  r0 ^ r1 -> r1                     (q0, 2) at day 4; (q1, 2); (q2, 4): 1 -> 3 by row 7, 3 -> 4 by row 5
#   5  id ^ id -> r1                     every query of r1 reaches its subject, windows or not: (q0, 0) (q1, 0) (q2, 1) (q7, 0) (q8, 3)
#   6  r0[2-3d] ^ r1[0-1d] -> r1         day 4: row 2 (0 -> 1, lag 3), then row 4 (1 -> 2, lag 1): (q0, 2)
# q6 = (2, r0, day 4) and q9 = (0, r0, day 4) get nothing: rule 0 needs an r0 row of lag 0 or 1 in day 4's window (the r0 rows there
# have the lags 4, 3, 3), rule 2 a self-loop of lag 61..120 (it is 4); q7 (day 122) and q8 (day 0) have empty windows and fire through
# the identity rule only.
HAND_ORDER = [0, 3, 6, 1, 2, 4, 5]
HAND_QUERIES = np.array([[0, 1, 4], [0, 1, 123], [1, 1, 123], [0, 0, 1], [0, 0, 123], [1, 0, 123], [2, 0, 4], [0, 1, 122], [3, 1, 0],
                         [0, 0, 4]])
HAND_FIRING = [[(3, 1), (4, 1)], [], [(4, 1), (5, 3)], [(1, 2)], [(0, 2), (1, 2), (2, 4)], [(0, 0), (1, 0), (2, 1), (7, 0), (8, 3)],
               [(0, 2)]]
HAND_BODY_PAIRS = [2, 0, 2, 1, 3, 12, 1]                 # xrule_ground_ref.HAND_ALL[HAND_ORDER, 0]
HAND_WEIGHT = np.array([0.5, 0.25, 0.75, 0.125, 0.625, 0.375, 0.875], np.float32)      # distinct, all exact in float32 and so are the misses


def hand_rules():
    """(head, body, lag_lo, lag_hi) of the hand data set, stably sorted by head."""
    from tests import xrule_ground_ref as X
    head, body, lo, hi = X.hand_rules()
    order, head, body, lo, hi = sort_by_head(head, body, lo, hi)
    assert order.tolist() == HAND_ORDER
    return head, body, lo, hi


def hand_expected(weight=HAND_WEIGHT):
    """The four arrays [10, 5] that HAND_FIRING and the fold give."""
    from tests.xrule_ground_ref import HAND_N_ENT
    weight = np.asarray(weight, np.float32)
    miss = miss_of(weight)
    best, surv, rule, fired = initial(len(HAND_QUERIES), HAND_N_ENT)
    for i, cells in enumerate(HAND_FIRING):
        for b, y in cells:
            fired[b, y] += 1
            surv[b, y] = np.float32(surv[b, y] * miss[i])
            if weight[i] > best[b, y]:
                best[b, y], rule[b, y] = weight[i], i
    return best, surv, rule, fired
