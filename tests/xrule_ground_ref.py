"""Host references of engine.xrule_ground (rg_xrule_ground) in numpy: the four counts of an extrapolation rule (head h, body
(r_1, [lo_1, hi_1)) .. (r_L, [lo_L, hi_L))) over the pairs ((x, t), y) with (x, t) in an anchor set - an entity and a query day - on
the forecasting model's data: rows data[j] = (s, r, o, ts) sorted by time, row_day[j] = ts // granularity, and per query day t the
forward's row window [win_lo[t], win_hi[t]) = [off[max(t - 120, 0)], off[t]) with the reference's offsets as they are (windows()).

A step (r, [lo, hi)) admits the data row j = (u, r, v) at day t iff win_lo[t] <= j < win_hi[t] and lo <= t - row_day[j] < hi; the
identity relation n_rel (the model's n_rel_true) stands for the self-loops, admitted at day t iff lo <= min(t, loop_window) < hi.
head(x, y | t) iff a data row (x, h, y) has row_day == t.  A repeated row counts once.

    windows(off)            (win_lo, win_hi) of every query day
    default_anchors(...)    the distinct (subject, day) of the data rows, sorted by (day, entity)
    counts_dense(...)       the definition, literally: per anchor day and step one dense boolean n_ent x n_ent matrix of the admitted
                            rows, then X <- (X.astype(np.int64) @ M) > 0 on the anchors of that day
    counts(...)             the same sets by expanding edge lists, day by day: out[v] |= X[u] over the admitted rows (u, v), entity-major
                            with the day's anchors for columns.  The dense form is slow beyond a few hundred anchors, so the larger
                            cases use this one; tests/test_xrule_ground_ref.py holds the two equal where both are cheap.

Both return int64 [R, 4] = (body_pairs, hits, pca_body_pairs, head_pairs), and both take the anchors in any order (counts are sums).
"""
import numpy as np

from tests.rule_ground_ref import _four

WINDOW = 120
ANY_HI = 2 ** 31 - 1                       # [0, ANY_HI) is any lag
DEFAULT_LAG_EDGES = (2, 4, 8, 15, 31, 61, 121)


def windows(off, window=WINDOW):
    off = np.asarray(off, np.int64)
    t = np.arange(len(off))
    return off[np.maximum(t - window, 0)], off[t]


def offsets(row_day):
    """extrapolation.get_time_offset_list on days: off[t + 1] = the index of the last row of day t, 0 where the day has none."""
    row_day = np.asarray(row_day, np.int64)
    off = np.zeros(int(row_day.max()) + 2, np.int64)
    off[row_day + 1] = np.arange(len(row_day))
    return off


def default_anchors(data, row_day, n_ent):
    data, row_day = np.asarray(data, np.int64).reshape(-1, 4), np.asarray(row_day, np.int64)
    key = np.unique(row_day * n_ent + data[:, 0])
    return np.stack([key % n_ent, key // n_ent], 1)


def bin_ranges(bins, lag_edges=DEFAULT_LAG_EDGES):
    """(lag_lo, lag_hi) of lag bins: bin b of profile.lag_bins, b = len(lag_edges) + 1 for ANY."""
    first = np.array((0,) + tuple(lag_edges) + (0,), np.int64)
    last = np.array(tuple(lag_edges) + (ANY_HI, ANY_HI), np.int64)
    bins = np.asarray(bins, np.int64)
    return first[bins], last[bins]


def _anchors(data, row_day, n_ent, n_day, anchors):
    a = default_anchors(data, row_day, n_ent) if anchors is None else np.asarray(anchors, np.int64).reshape(-1, 2)
    assert len(np.unique(a, axis=0)) == len(a)
    assert len(a) == 0 or (a.min() >= 0 and a[:, 0].max() < n_ent and a[:, 1].max() < n_day)
    return a[np.lexsort((a[:, 0], a[:, 1]))]


def _loop_ok(t, lo, hi, loop_window):
    return lo <= min(t, loop_window) < hi


def counts_dense(n_ent, n_rel, data, row_day, win_lo, win_hi, head, body, lag_lo, lag_hi, anchors=None, loop_window=WINDOW):
    data, row_day = np.asarray(data, np.int64).reshape(-1, 4), np.asarray(row_day, np.int64)
    a = _anchors(data, row_day, n_ent, len(win_lo), anchors)
    seed = np.zeros((len(a), n_ent), dtype=bool)
    seed[np.arange(len(a)), a[:, 0]] = True
    days = np.unique(a[:, 1])

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

    def hop(X, r, lo, hi):
        out = np.zeros_like(X)
        for t in days.tolist():
            at = a[:, 1] == t
            out[at] = (X[at].astype(np.int64) @ matrix(t, r, lo, hi)) > 0
        return out

    def head_of(h):
        H = np.zeros_like(seed)
        for t in days.tolist():
            M = np.zeros((n_ent, n_ent), dtype=bool)
            rows = data[(row_day == t) & (data[:, 1] == h)]
            M[rows[:, 0], rows[:, 2]] = True
            at = a[:, 1] == t
            H[at] = (seed[at].astype(np.int64) @ M) > 0
        return H

    out = []
    for h, b, los, his in zip(*(np.asarray(x).tolist() for x in (head, body, lag_lo, lag_hi))):
        X = seed
        for r, lo, hi in zip(b, los, his):
            X = hop(X, r, lo, hi)
        out.append(_four(X, head_of(h)))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def counts(n_ent, n_rel, data, row_day, win_lo, win_hi, head, body, lag_lo, lag_hi, anchors=None, loop_window=WINDOW):
    data, row_day = np.asarray(data, np.int64).reshape(-1, 4), np.asarray(row_day, np.int64)
    a = _anchors(data, row_day, n_ent, len(win_lo), anchors)
    rules = [np.asarray(x, np.int64) for x in (head, body, lag_lo, lag_hi)]
    R = len(rules[0])
    out = np.zeros((R, 4), np.int64)
    s, rel, o = data[:, 0], data[:, 1], data[:, 2]

    def expand(X, u, v):                                              # X bool [n_ent, S_t]: out[v] |= X[u] over the edges (u, v)
        res = np.zeros_like(X)
        if len(u):
            order = np.argsort(v, kind="stable")
            tails, starts = np.unique(v[order], return_index=True)
            res[tails] = np.logical_or.reduceat(X[u[order]], starts, axis=0)
        return res

    for t in np.unique(a[:, 1]).tolist():
        ents = a[a[:, 1] == t, 0]
        seed = np.zeros((n_ent, len(ents)), dtype=bool)
        seed[ents, np.arange(len(ents))] = True
        idx = np.arange(int(win_lo[t]), max(int(win_hi[t]), int(win_lo[t])))
        lag = t - row_day[idx]
        today = np.nonzero(row_day == t)[0]
        heads = {}
        for i in range(R):
            h, b, los, his = (x[i] for x in rules)
            X = seed
            for r, lo, hi in zip(b.tolist(), los.tolist(), his.tolist()):
                if r == n_rel:
                    X = X if _loop_ok(t, lo, hi, loop_window) else np.zeros_like(X)
                else:
                    e = idx[(rel[idx] == r) & (lag >= lo) & (lag < hi)]
                    X = expand(X, s[e], o[e])
            h = int(h)
            if h not in heads:
                e = today[rel[today] == h]
                heads[h] = expand(seed, s[e], o[e])
            H = heads[h]
            out[i] += [X.sum(), (X & H).sum(), X[:, H.any(0)].sum(), H.sum()]
    return out


def random_rules(rng, n, n_rela, lag_edges=DEFAULT_LAG_EDGES, max_hops=3):
    """{L: (head [n_L], body [n_L, L], lag_lo [n_L, L], lag_hi [n_L, L])} for L in 1..max_hops, n rules in all: relations over all
    ids (the identity n_rela - 1 included, under every bin: a self-loop has a lag too), heads among the others, every second step
    ANY on average and the others uniform over the bins."""
    out = {}
    n_bins = len(lag_edges) + 1
    for L in range(1, max_hops + 1):
        k = n // max_hops + (1 if L <= n % max_hops else 0)
        bins = np.where(rng.integers(0, 2, (k, L)) == 0, n_bins, rng.integers(0, n_bins, (k, L)))
        out[L] = (rng.integers(0, n_rela - 1, k), rng.integers(0, n_rela, (k, L))) + bin_ranges(bins, lag_edges)
    return out


def graph_rows(data, n_ent, n_rel):
    """The rows extrapolation.T_RED_GNN builds its device graph from: the self-loops (e, n_rel, e, n_data), then the data rows with
    their own row index as time field.  int32 [n_ent + n_data, 4]; the graph has n_rel + 1 relation rows and n_data + 1 time ids."""
    data = np.asarray(data, np.int64).reshape(-1, 4)
    ent = np.arange(n_ent)
    loops = np.stack([ent, np.full(n_ent, n_rel), ent, np.full(n_ent, len(data))], 1)
    return np.concatenate([loops, np.concatenate([data[:, :3], np.arange(len(data))[:, None]], 1)], 0).astype(np.int32)


# ---- a data set small enough to count by hand -----------------------------------------------------------------------
# 5 entities, relations 0 = r0, 1 = r1, 2 = r2 (no row), 3 = the identity; one time unit a day.  Rows j: (s, r, o, day):
HAND_N_ENT, HAND_N_REL = 5, 3
HAND_DATA = np.array([[0, 0, 1, 0], [1, 1, 2, 0],                    # 0, 1     day 0
                      [0, 0, 1, 1], [2, 0, 3, 1],                    # 2, 3     day 1: (0, r0, 1) once more
                      [1, 1, 2, 3], [3, 1, 4, 3],                    # 4, 5     day 3 (day 2 has no row)
                      [0, 1, 2, 4], [1, 0, 3, 4],                    # 6, 7     day 4
                      [0, 0, 1, 122], [2, 1, 4, 122],                # 8, 9     day 122
                      [0, 1, 4, 123], [1, 1, 2, 123]])               # 10, 11   day 123
HAND_ROW_DAY = HAND_DATA[:, 3]
# off[t + 1] = the last row of day t: off[1] = 1, off[2] = 3, off[3] = 0 (no row on day 2), off[4] = 5, off[5] = 7, off[6..122] = 0,
# off[123] = 9, off[124] = 11; n_day = 125.  The windows [off[max(t - 120, 0)], off[t]) of the days that have rows:
#   day 0 [0, 0) empty   day 1 [0, 1): row 0 (row 1, the last of day 0, is left out)   day 3 [0, 0) empty: it follows a day without rows
#   day 4 [0, 5): rows 0..4, lags 4 4 3 3 1 (row 5, the last of day 3, is left out)   day 122 [off[2], off[122]) = [3, 0) empty
#   day 123 [off[3], off[123]) = [0, 9): day 2 has no row, so the window starts at row 0: rows 0..8 with lags 123 123 122 122 120 120
#   119 119 1 - four of them above 120
HAND_OFF = np.array([0, 1, 3, 0, 5, 7] + [0] * 117 + [9, 11])
# default anchors (subject, day): day 0 {0, 1}, day 1 {0, 2}, day 3 {1, 3}, day 4 {0, 1}, day 122 {0, 2}, day 123 {0, 1}: 12 in all
HAND_ANCHORS = np.array([[0, 0], [1, 0], [0, 1], [2, 1], [1, 3], [3, 3], [0, 4], [1, 4], [0, 122], [2, 122], [0, 123], [1, 123]])
# heads on the anchors' own days: r0 ((0,0),1) ((0,1),1) ((2,1),3) ((1,4),3) ((0,122),1): 5;  r1 ((1,0),2) ((1,3),2) ((3,3),4) ((0,4),2)
# ((2,122),4) ((0,123),4) ((1,123),2): 7
HAND_HEAD = np.array([0, 1, 1, 0, 1, 1, 0])
HAND_BODY = np.array([[3, 0],     # id ^ r0[0-1d] -> r0: ((0,1),1) by row 0 and ((0,123),1) by row 8; (0, r0, 1) is a fact of day 1, not of day 123
                      [0, 1],     # r0[121+] ^ r1 -> r1: only day 123 sees lags above 120: rows 0, 2 (0 -> 1), 3 (2 -> 3); then 1 -> 2: ((0,123),2)
                      [0, 1],     # r0 ^ r1 -> r1: ((0,4),2), a fact of day 4; ((0,123),2); ((1,123),4) by rows 7 and 5; all three anchors have an r1 fact
                      [2, 0],     # r2 ^ r0 -> r0: a relation without rows
                      [3, 3],     # id ^ id -> r1: every anchor reaches itself: 12; the 7 anchors with an r1 fact
                      [0, 1],     # r0[2-3d] ^ r1[0-1d] -> r1: day 4: rows 2 (0 -> 1), 3 (2 -> 3), then row 4 (1 -> 2): ((0,4),2), a fact
                      [3, 0]])    # id[61-120d] ^ r0 -> r0: a self-loop's lag is min(t, 120): days 122 (empty window) and 123: ((0,123),1), ((1,123),3)
HAND_BINS = np.array([[8, 0], [7, 8], [8, 8], [8, 8], [8, 8], [1, 0], [6, 8]])          # 8 = ANY, 7 = 121+
HAND_ALL = np.array([[2, 1, 1, 5], [1, 0, 1, 7], [3, 1, 3, 7], [0, 0, 0, 5], [12, 0, 7, 7], [1, 1, 1, 7], [2, 0, 0, 5]])
# a subset, given out of day order, with (1, 1) and (2, 4), which are no default anchors.  From (2, 4) row 3 leads to 3, and the only
# r1 row from 3 is row 5, the last row of day 3, which day 4's window leaves out: rules 2 and 5 ground nothing there
HAND_SUBSET = np.array([[2, 4], [0, 123], [1, 1]])
HAND_SUB = np.array([[1, 0, 0, 0], [1, 0, 1, 1], [1, 0, 1, 1], [0, 0, 0, 0], [3, 0, 1, 1], [0, 0, 0, 1], [1, 0, 0, 0]])


def hand_rules():
    return (HAND_HEAD, HAND_BODY) + bin_ranges(HAND_BINS)
