"""The host side of applying extrapolation rules (no GPU): engine.check_xrule_apply, which runs before anything touches a device, the
query layout rg_xrule_apply takes (the sort, q_ptr, day_ptr, day_of, day_pos) on a typed-in example, explain.rule_weights on a
LagRuleQuality built by hand, the day cut of rule_evaluate's default anchors, and the new C symbol in the header, in _lib.SYMBOLS
and in the library."""
import os
import re
import types

import numpy as np
import pytest
import torch

from red_gnn_amd import engine
from red_gnn_amd.explain import LagRuleQuality, LagRuleTable, anchors_before, rule_weights
from red_gnn_amd.profile import DEFAULT_LAG_EDGES as EDGES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANY_HI = 2 ** 31 - 1
N_DATA = 6


def _valid():
    g = types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=N_DATA + 1)            # no handle, no device: validation never asks for them
    return dict(graph=g, head=np.array([0, 1]), body=np.array([[0, 3], [2, 1]]), lag_lo=np.array([[0, 0], [2, 121]]),
                lag_hi=np.array([[2, ANY_HI], [4, ANY_HI]]), weight=np.array([0.5, 1.0], np.float32), subs=np.array([0, 4, 4]),
                rels=np.array([1, 0, 3]), days=np.array([5, 0, 2]), row_day=np.array([0, 0, 1, 3, 3, 4]), win_lo=np.zeros(6, np.int64),
                win_hi=np.array([0, 1, 2, 0, 4, 5]))


def test_check_xrule_apply_errors():
    cases = [
        ("head must be", dict(body=np.array([[0, 3]]))),
        ("head must be", dict(lag_lo=np.array([[0], [2]]))),
        ("head must be", dict(lag_hi=np.array([[2, ANY_HI]]))),
        ("must be int32 or int64", dict(lag_hi=np.array([[2.0, 3.0], [4.0, 5.0]]))),
        ("must be int32 or int64", dict(subs=np.array([0.0, 4.0, 4.0]))),
        ("must be int32 or int64", dict(days=np.array([5.0, 0.0, 2.0]))),
        ("body length 33", dict(body=np.zeros((2, 33), np.int64), lag_lo=np.zeros((2, 33), np.int64), lag_hi=np.ones((2, 33), np.int64))),
        ("not the extrapolation layout", dict(graph=types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=0))),       # a static graph
        ("not the extrapolation layout", dict(graph=types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=12))),      # an interpolation graph
        ("not the extrapolation layout", dict(row_day=np.array([0, 0, 1, 3, 3]))),
        (r"win_lo and win_hi must be \[n_day\]", dict(win_lo=np.zeros(5, np.int64))),
        ("window bound out of range", dict(win_hi=np.array([0, 1, 2, 0, 4, 7]))),
        ("loop_window must be", dict(loop_window=-1)),
        (r"relation id out of range 0\.\.3", dict(body=np.array([[0, 4], [2, 1]]))),
        (r"relation id out of range 0\.\.3", dict(head=np.array([-1, 1]))),
        ("lag range out of order", dict(lag_lo=np.array([[2, 0], [2, 121]]))),
        (r"row_day out of range 0\.\.5", dict(row_day=np.array([0, 0, 1, 3, 3, 6]))),
        (r"head must be non-decreasing \(rule 1 has head 0 after 1\)", dict(head=np.array([1, 0]))),
        (r"weight must be a float array \[R\]", dict(weight=np.array([1, 1]))),
        (r"weight must be a float array \[R\]", dict(weight=np.array([0.5], np.float32))),
        (r"weights must be finite and in \(0, 1\]", dict(weight=np.array([0.5, 0.0]))),
        (r"weights must be finite and in \(0, 1\]", dict(weight=np.array([0.5, 1.5]))),
        (r"weights must be finite and in \(0, 1\]", dict(weight=np.array([np.nan, 0.5]))),
        ("need one relation and one day per subject", dict(rels=np.array([1, 0]))),
        ("need one relation and one day per subject", dict(days=np.array([[5, 0, 2]]))),
        (r"subject id out of range 0\.\.4", dict(subs=np.array([0, 5, 4]))),
        (r"subject id out of range 0\.\.4", dict(subs=np.array([0, -1, 4]))),
        (r"query relation id out of range 0\.\.3", dict(rels=np.array([1, 0, 4]))),
        (r"query day out of range 0\.\.5 \(got 0\.\.6\)", dict(days=np.array([6, 0, 2]))),
        (r"query day out of range 0\.\.5", dict(days=np.array([5, -1, 2]))),
    ]
    for match, change in cases:
        kw = _valid()
        kw.update(change)
        with pytest.raises(ValueError, match="xrule_apply: .*" + match):
            engine.check_xrule_apply(**kw)
    for bad in (-1, 1.5, True):                                                      # the budget is checked first, before any device
        with pytest.raises(ValueError, match="xrule_apply: scratch_bytes must be"):
            engine.xrule_apply(scratch_bytes=bad, **_valid())
    kw = _valid()
    kw["body"], kw["days"] = torch.as_tensor(kw["body"]), torch.as_tensor(kw["days"])
    out = engine.check_xrule_apply(**kw)
    assert len(out) == 11 and all(x.dtype == np.int32 for x in out[:4] + out[5:]) and out[4].dtype == np.float32
    assert out[3].tolist() == _valid()["lag_hi"].tolist() and out[7].tolist() == [5, 0, 2] and out[4].tolist() == [0.5, 1.0]
    empty = dict(_valid(), subs=np.zeros(0, np.int64), rels=np.zeros(0, np.int64), days=np.zeros(0, np.int64))
    assert engine.check_xrule_apply(**empty)[5].shape == (0,)                        # no query is fine


def test_query_layout_typed_in():
    # 5 relation rows; relation 2 has no query between 1 and 3 that have, relation 0 and 4 have none either.  Queries b = 0..8 as
    # (relation, day); (3, 7) is stated three times (b = 1, 4, 8), (1, 9) twice (b = 3, 6)
    rels = np.array([3, 3, 1, 1, 3, 1, 1, 3, 3])
    days = np.array([9, 7, 4, 9, 7, 0, 9, 2, 7])
    order, q_ptr, day_ptr, day_of, day_pos = engine.xrule_query_layout(rels, days, 5, 10)
    # sorted stably by (relation, day): relation 1: (1,0) b5, (1,4) b2, (1,9) b3 b6;  relation 3: (3,2) b7, (3,7) b1 b4 b8, (3,9) b0
    assert order.tolist() == [5, 2, 3, 6, 7, 1, 4, 8, 0]
    assert q_ptr.tolist() == [0, 0, 4, 4, 9, 9]
    assert day_ptr.tolist() == [0, 0, 3, 3, 6, 6]
    assert day_of.tolist() == [0, 4, 9, 2, 7, 9]
    assert day_pos.tolist() == [0, 1, 2, 4, 5, 8, 9]
    assert all(x.dtype == np.int32 for x in (q_ptr, day_ptr, day_of, day_pos))
    # the end of a relation's last entry is the first position of the next relation that has queries
    assert day_pos[day_ptr[2]] == q_ptr[2] == q_ptr[3] and day_pos[-1] == len(rels)
    # entry k of relation h owns the columns [day_pos[k] - q_ptr[h], day_pos[k + 1] - q_ptr[h])
    assert [(int(day_pos[k] - q_ptr[3]), int(day_pos[k + 1] - q_ptr[3])) for k in range(3, 6)] == [(0, 1), (1, 4), (4, 5)]
    none = engine.xrule_query_layout(rels[:0], days[:0], 5, 10)
    assert none[1].tolist() == [0] * 6 and none[2].tolist() == [0] * 6 and none[3].shape == (0,) and none[4].tolist() == [0]
    # random: every entry's positions hold exactly its (relation, day), entries ascend inside a relation
    rng = np.random.default_rng(5)
    r, t = rng.integers(0, 7, 300), rng.choice([0, 3, 4, 50, 51, 219], 300)
    order, q_ptr, day_ptr, day_of, day_pos = engine.xrule_query_layout(r, t, 7, 220)
    assert sorted(order.tolist()) == list(range(300)) and day_pos[-1] == 300 and day_ptr[-1] == len(day_of)
    for h in range(7):
        k0, k1 = day_ptr[h], day_ptr[h + 1]
        assert (np.diff(day_of[k0:k1]) > 0).all() and (k0 == k1 or (day_pos[k0] == q_ptr[h] and day_pos[k1] == q_ptr[h + 1]))
        for k in range(k0, k1):
            at = order[day_pos[k]:day_pos[k + 1]]
            assert len(at) and (r[at] == h).all() and (t[at] == day_of[k]).all() and (np.diff(at) > 0).all()      # stable


def test_rule_weights_on_a_lag_rule_quality():
    head = torch.tensor([0, 0, 0, 1, 1])
    body = torch.tensor([[6, 0], [0, 6], [2, 3], [6, 1], [1, 3]])
    bins = torch.tensor([[8, 0], [0, 8], [0, 2], [8, 1], [8, 8]])
    one = torch.ones(5, dtype=torch.int64)
    table = LagRuleTable(head, body, bins, one, one.clone(), EDGES, 6)
    t = lambda *x: torch.tensor(x, dtype=torch.int64)
    q = LagRuleQuality(table, body_pairs=t(8, 10, 4, 3, 0), hits=t(8, 5, 1, 3, 0), pca_body_pairs=t(8, 5, 2, 3, 0), head_pairs=t(8, 8, 8, 3, 8),
                       n_anchors=7)
    rows, w = rule_weights(q)
    # row 0, the head relation as the only step, is kept: no window holds a fact of the query day, so no rule of this family is trivial
    assert rows.tolist() == [0, 1, 2, 3] and w.dtype == np.float32 and w.tolist() == [1.0, 0.5, 0.25, 1.0]
    assert rule_weights(q, drop_trivial=False)[0].tolist() == [0, 1, 2, 3]
    rows, w = rule_weights(q, by="pca_confidence", min_hits=2)
    assert rows.tolist() == [0, 1, 3] and w.tolist() == [1.0, 1.0, 1.0]
    rows, w = rule_weights(q, laplace=2.0)
    assert rows.tolist() == [0, 1, 2, 3] and np.array_equal(w, np.array([8 / 10, 5 / 12, 1 / 6, 3 / 5]).astype(np.float32))
    assert rule_weights(q, min_hits=0)[0].tolist() == [0, 1, 2, 3]                   # hits 0 has weight 0: never kept
    with pytest.raises(ValueError, match="by must be"):
        rule_weights(q, by="hits")
    with pytest.raises(ValueError, match="quality must be"):
        rule_weights(table)


def test_the_day_cut_of_the_default_anchors():
    a = np.array([[2, 0], [0, 1], [0, 3], [2, 3], [4, 4], [1, 7]])
    assert anchors_before(a, 4).tolist() == [[2, 0], [0, 1], [0, 3], [2, 3]]        # the query day's own anchors are left out
    assert anchors_before(a, 3).tolist() == [[2, 0], [0, 1]] and anchors_before(a, 100).tolist() == a.tolist()
    with pytest.raises(ValueError, match="rule_evaluate: no anchor lies before the earliest query day 0"):
        anchors_before(a, 0)
    with pytest.raises(ValueError, match="no anchor lies before"):
        anchors_before(a[:0], 5)


def test_header_and_binding_carry_the_symbol():
    from red_gnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redgnn.h")).read(), flags=re.S)
    assert re.search(r"\brg_xrule_apply\s*\(", text) and "rg_xrule_apply" in _lib.SYMBOLS
    assert "rg_xrule_apply_scratch_bytes" not in text                   # the scratch is rg_rule_apply_scratch_bytes': no new size function
    L = _lib.lib()
    assert hasattr(L, "rg_xrule_apply") and len(L.rg_xrule_apply.argtypes) == 33
    assert L.rg_version() == 12
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: NULL graph"):
        _lib.check(L.rg_xrule_apply(*([None] * 7), 1, 1, 0, None, 1, None, None, 1, 120, *([None] * 6), 1, 1, None, 1, None, 3,
                                    *([None] * 5)))
