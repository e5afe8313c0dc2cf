"""tests/xrule_apply_ref.py against itself, against the typed-in cells of the hand data set and against the counts of
tests/xrule_ground_ref.py (no GPU)."""
import numpy as np

from tests import xrule_apply_ref as XA
from tests import xrule_ground_ref as X


def _hand():
    lo, hi = X.windows(X.HAND_OFF)
    return (X.HAND_N_ENT, X.HAND_N_REL, X.HAND_DATA, X.HAND_ROW_DAY, lo, hi)


def test_hand_cells():
    data, rules = _hand(), XA.hand_rules()
    assert rules[0].tolist() == [0, 0, 0, 1, 1, 1, 1] and np.array_equal(rules[1], X.HAND_BODY[XA.HAND_ORDER])
    q = XA.HAND_QUERIES
    assert [tuple(x) for x in q.tolist()] == [(0, 1, 4), (0, 1, 123), (1, 1, 123), (0, 0, 1), (0, 0, 123), (1, 0, 123), (2, 0, 4),
                                              (0, 1, 122), (3, 1, 0), (0, 0, 4)]
    args = data + rules + (XA.HAND_WEIGHT, q[:, 0], q[:, 1], q[:, 2])
    exp = XA.hand_expected()
    dense = XA.apply_dense(*args)
    assert XA.same(dense, exp)
    assert XA.same(XA.cells_to_dense(XA.apply_cells(*args), len(q), X.HAND_N_ENT), exp)
    # every rule alone: exactly its typed-in cells
    for i, cells in enumerate(XA.HAND_FIRING):
        one = XA.apply_dense(*data, *(x[i:i + 1] for x in rules), XA.HAND_WEIGHT[i:i + 1], q[:, 0], q[:, 1], q[:, 2])[3]
        assert [tuple(c) for c in np.argwhere(one).tolist()] == sorted(cells), i
    best, surv, rule, fired = exp
    assert not fired[6].any() and not fired[9].any()                         # q6 and q9 get nothing
    for b, y in ((7, 0), (8, 3)):                                            # empty windows: the identity rule alone
        assert np.argwhere(fired[b]).tolist() == [[y]] and rule[b, y] == 5 and fired[b, y] == 1
        assert X.windows(X.HAND_OFF)[0][q[b, 2]] >= X.windows(X.HAND_OFF)[1][q[b, 2]]
    w, miss = XA.HAND_WEIGHT, XA.miss_of(XA.HAND_WEIGHT)
    assert len(set(w.tolist())) == 7
    # cell (q0, 2): rules 4 and 6
    assert fired[0, 2] == 2 and surv[0, 2] == np.float32(miss[4] * miss[6])
    assert best[0, 2] == max(w[4], w[6]) == w[6] and rule[0, 2] == 6
    # cell (q4, 1): rules 0 and 2
    assert fired[4, 1] == 2 and surv[4, 1] == np.float32(miss[0] * miss[2])
    assert best[4, 1] == max(w[0], w[2]) == w[2] and rule[4, 1] == 2
    # the larger weight first: the later rule does not displace it
    swapped = w.copy()
    swapped[[4, 6]] = w[[6, 4]]
    sw = XA.apply_dense(*data, *rules, swapped, q[:, 0], q[:, 1], q[:, 2])
    assert sw[2][0, 2] == 4 and sw[0][0, 2] == w[6] and sw[1][0, 2] == surv[0, 2]
    assert XA.same(sw, XA.hand_expected(swapped))


def test_hand_agrees_with_the_grounding_counts():
    """With the 12 default anchors as queries under a rule's head, the cells it fires for are its body pairs."""
    data, rules = _hand(), XA.hand_rules()
    assert X.HAND_ALL[XA.HAND_ORDER, 0].tolist() == XA.HAND_BODY_PAIRS == [2, 0, 2, 1, 3, 12, 1]
    a = X.HAND_ANCHORS
    for i in range(7):
        one = tuple(x[i:i + 1] for x in rules)
        rels = np.full(len(a), one[0][0])
        for form in (XA.apply_dense(*data, *one, [0.5], a[:, 0], rels, a[:, 1])[3],
                     XA.cells_to_dense(XA.apply_cells(*data, *one, [0.5], a[:, 0], rels, a[:, 1]), len(a), X.HAND_N_ENT)[3]):
            assert int(form.sum()) == XA.HAND_BODY_PAIRS[i], i
    assert np.array_equal(X.counts_dense(*data, *rules)[:, 0], XA.HAND_BODY_PAIRS)


def _small(seed=3, n_ent=30, n_rel=3, n_day=140, m=400):
    """Random rows over 140 days with days without rows, so that windows are empty, start at row 0 and hold lags above 120."""
    rng = np.random.default_rng(seed)
    day = np.sort(rng.choice(np.setdiff1d(np.arange(n_day), [2, 15, 16, 70]), m))
    data = np.column_stack([rng.integers(0, n_ent, m), rng.integers(0, n_rel, m), rng.integers(0, n_ent, m), day])
    off = X.offsets(day)
    lo, hi = X.windows(off)
    return n_ent, n_rel, data, day, lo, hi, rng


def test_the_references_agree_and_ranges_change_nothing():
    n_ent, n_rel, data, row_day, lo, hi, rng = _small()
    n_day = len(lo)
    assert (lo[1:] > hi[1:]).any() and ((lo == 0) & (hi > 0) & (np.arange(n_day) > 121)).any()      # not monotone; from row 0 with old rows
    B = 80
    subs, rels = rng.integers(0, n_ent, B), rng.integers(0, n_rel, B)
    days = rng.choice([0, 3, 16, 17, 71, 90, 125, 136, 137, n_day - 1], B)
    subs[1], rels[1], days[1] = subs[0], rels[0], days[0]               # a query stated twice
    base = (n_ent, n_rel, data, row_day, lo, hi)
    some2 = False
    for L, r in X.random_rules(rng, 36, n_rel + 1).items():
        order, head, body, l0, l1 = XA.sort_by_head(*r)
        weight = rng.integers(1, 257, len(head)).astype(np.float32) / np.float32(256)
        q = (subs, rels, days)
        dense = XA.apply_dense(*base, head, body, l0, l1, weight, *q)
        cells = XA.apply_cells(*base, head, body, l0, l1, weight, *q)
        assert XA.same(XA.cells_to_dense(cells, B, n_ent), dense)
        assert XA.same(XA.apply_lists(*base, head, body, l0, l1, weight, *q), dense)
        assert (dense[3] > 0).sum() > 20, L
        assert np.array_equal(dense[0][0], dense[0][1]) and np.array_equal(dense[3][0], dense[3][1])
        some2 |= bool((dense[3] >= 2).any())
        state_d, state_c, state_l = None, None, None
        for r0, r1 in ((0, 5), (5, 6), (6, len(head))):                 # rules cut into ranges, carried through state and rule_base
            part = (head[r0:r1], body[r0:r1], l0[r0:r1], l1[r0:r1], weight[r0:r1]) + q
            state_d = XA.apply_dense(*base, *part, state=state_d, rule_base=r0)
            state_c = XA.apply_cells(*base, *part, state=state_c, rule_base=r0)
            state_l = XA.apply_lists(*base, *part, state=state_l, rule_base=r0)
        assert XA.same(state_d, dense) and XA.same(XA.cells_to_dense(state_c, B, n_ent), dense) and XA.same(state_l, dense)
        # the grounding reference counts the same pairs: distinct (subject, day) of one relation's queries as anchors
        for i in range(0, len(head), 5):
            at = rels == head[i]
            anchors = np.unique(np.column_stack([subs[at], days[at]]), axis=0)
            one = (head[i:i + 1], body[i:i + 1], l0[i:i + 1], l1[i:i + 1])
            got = XA.apply_dense(*base, *one, [0.5], anchors[:, 0], np.full(len(anchors), head[i]), anchors[:, 1])[3]
            assert int(got.sum()) == X.counts(*base, *one, anchors)[0, 0]
    assert some2
    # another loop window moves the self-loops' lag
    idn = (np.array([0]), np.array([[n_rel]]), np.array([[4]]), np.array([[8]]))
    for lw in (120, 5):                                                  # with 5 every query day from 4 on has the lag 4 or 5
        got = XA.apply_dense(*base, *idn, [0.5], subs, rels, days, loop_window=lw)[3]
        want = ((rels == 0) & (np.minimum(days, lw) >= 4) & (np.minimum(days, lw) < 8)).sum()
        assert got.sum() == want and (want > 0) == (lw == 5)
        assert XA.same(XA.cells_to_dense(XA.apply_cells(*base, *idn, [0.5], subs, rels, days, loop_window=lw), B, n_ent),
                       XA.apply_dense(*base, *idn, [0.5], subs, rels, days, loop_window=lw))
