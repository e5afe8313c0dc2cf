"""tests/xrule_ground_ref.py against itself (no GPU): the dense definition and the edge-list form agree with the counts typed in for the
hand data set and with each other on the fixture the GPU tests use, and the counts keep their order."""
import numpy as np
import pytest

from tests import extrap_ref as ER
from tests import xrule_ground_ref as X


def _invariants(c):
    assert (c >= 0).all()
    assert (c[:, 1] <= c[:, 2]).all() and (c[:, 2] <= c[:, 0]).all() and (c[:, 1] <= c[:, 3]).all()


def _hand(fn, anchors=None):
    lo, hi = X.windows(X.HAND_OFF)
    return fn(X.HAND_N_ENT, X.HAND_N_REL, X.HAND_DATA, X.HAND_ROW_DAY, lo, hi, *X.hand_rules(), anchors)


def test_hand_data_set_is_what_its_comments_say():
    assert np.array_equal(X.offsets(X.HAND_ROW_DAY), X.HAND_OFF) and len(X.HAND_OFF) == 125
    lo, hi = X.windows(X.HAND_OFF)
    assert [(int(lo[t]), int(hi[t])) for t in (0, 1, 3, 4, 122, 123)] == [(0, 0), (0, 1), (0, 0), (0, 5), (3, 0), (0, 9)]
    assert X.HAND_OFF[3] == 0 and X.HAND_OFF[123 - 120] == 0                   # a day without rows; day 123's window starts at row 0
    assert (123 - X.HAND_ROW_DAY[:9]).max() == 123                              # ... and holds lags above 120
    assert np.array_equal(X.default_anchors(X.HAND_DATA, X.HAND_ROW_DAY, X.HAND_N_ENT), X.HAND_ANCHORS)
    assert (X.HAND_DATA[0, :3] == X.HAND_DATA[2, :3]).all() and X.HAND_ROW_DAY[0] != X.HAND_ROW_DAY[2]      # a fact repeated on two days
    assert not (X.HAND_DATA[:, 1] == 2).any()                                   # r2 has no row
    lag_lo, lag_hi = X.hand_rules()[2:]
    assert lag_lo[0].tolist() == [0, 0] and lag_hi[0].tolist() == [X.ANY_HI, 2]
    assert (lag_lo[1, 0], lag_hi[1, 0]) == (121, X.ANY_HI) and (lag_lo[6, 0], lag_hi[6, 0]) == (61, 121)


@pytest.mark.parametrize("fn", [X.counts_dense, X.counts])
def test_hand_counts(fn):
    assert np.array_equal(_hand(fn), X.HAND_ALL)
    assert np.array_equal(_hand(fn, X.HAND_ANCHORS[::-1]), X.HAND_ALL)          # the anchors in any order
    assert np.array_equal(_hand(fn, X.HAND_SUBSET), X.HAND_SUB)
    assert 0 < X.HAND_ALL[0, 1] < X.HAND_ALL[0, 0]                              # a rule that holds sometimes
    _invariants(X.HAND_ALL)
    _invariants(X.HAND_SUB)
    assert not _hand(fn, np.zeros((0, 2), np.int64)).any()
    # counts over disjoint anchor sets add
    assert np.array_equal(_hand(fn, X.HAND_ANCHORS[:5]) + _hand(fn, X.HAND_ANCHORS[5:]), X.HAND_ALL)


def test_forms_agree_on_the_fixture():
    data, _ = ER.make_case(32, 9)
    row_day = data[:, 3] // 24
    off = X.offsets(row_day)
    assert np.nonzero(off == 0)[0].tolist() == [0, 1, 51, 52, 121]
    lo, hi = X.windows(off)
    anchors = X.default_anchors(data, row_day, ER.N_ENT)
    assert len(anchors) == 4062
    # windows that start at row 0 long after day 0: the largest lag any window holds
    t = np.arange(len(off))
    assert max(int(d - row_day[lo[d]]) for d in t[lo < hi]) == 171
    rng = np.random.default_rng(5)
    part = anchors[np.sort(rng.permutation(len(anchors))[:300])]
    part = np.concatenate([part, anchors[anchors[:, 1] >= 171][:40]], 0)
    part = np.unique(part, axis=0)
    rules = X.random_rules(np.random.default_rng(3), 12, ER.N_REL + 1)
    some = 0
    for L, r in rules.items():
        a = X.counts(ER.N_ENT, ER.N_REL, data, row_day, lo, hi, *r, part)
        assert np.array_equal(a, X.counts_dense(ER.N_ENT, ER.N_REL, data, row_day, lo, hi, *r, part)), L
        _invariants(a)
        some += int((a[:, 0] > 0).sum())
    assert some >= 6
