"""tests/trule_apply_ref.py against itself and against typed-in cells (no GPU), the host validation of engine.trule_apply, which runs
before anything touches a device, explain.rule_weights on a TemporalRuleQuality built by hand, and the new C symbol in the header, in
_lib.SYMBOLS and in the library."""
import os
import re
import types

import numpy as np
import pytest
import torch

from red_gnn_amd.engine import check_trule_apply, trule_apply
from tests import rule_apply_ref as A
from tests import trule_apply_ref as TA
from tests import trule_ground_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(seed=4, n_ent=40, n_rel=3, n_time=6, m=150):
    """Random quadruples with inverses and identity rows (at the sentinel time n_time - 1), some facts at two times, one row twice."""
    rng = np.random.default_rng(seed)
    base = np.column_stack([rng.integers(0, n_ent, m), rng.integers(0, n_rel, m), rng.integers(0, n_ent, m), rng.integers(0, n_time, m)])
    again = base[:20].copy()
    again[:, 3] = (again[:, 3] + 1 + rng.integers(0, n_time - 1, 20)) % n_time
    base = np.concatenate([base, again, base[:1]], 0)
    ent = np.arange(n_ent)
    n_rela = 2 * n_rel + 1
    quads = np.concatenate([base, np.column_stack([base[:, 2], base[:, 1] + n_rel, base[:, 0], base[:, 3]]),
                            np.column_stack([ent, np.full(n_ent, n_rela - 1), ent, np.full(n_ent, n_time - 1)])], 0).astype(np.int64)
    return n_ent, n_rela, n_time, quads, rng


def _rules(rng, n, L, n_rela, heads):
    head = np.sort(rng.choice(heads, n))
    body = rng.integers(0, n_rela, (n, L))
    direc = np.where(rng.random((n, L)) < 0.5, 3, rng.integers(0, 3, (n, L)))
    weight = rng.integers(1, 257, n).astype(np.float32) / np.float32(256)
    return head, body, direc, weight


def test_hand_cells():
    quads = T.hand_quads()
    args = (T.HAND_N_ENT, T.HAND_N_RELA, T.HAND_N_TIME, quads, TA.HAND_HEAD, TA.HAND_BODY, TA.HAND_DIR, TA.HAND_WEIGHT,
            TA.HAND_SUBS, TA.HAND_RELS, TA.HAND_TIMES)
    exp = TA.hand_expected()
    assert A.same(TA.apply_dense(*args), exp)
    assert A.same(A.cells_to_dense(TA.apply_cells(*args), len(TA.HAND_SUBS), T.HAND_N_ENT), exp)
    best, surv, rule, fired = exp
    assert fired[0, 2] == 2 and rule[0, 2] == 3 and surv[0, 2] == np.float32(0.375)      # two typed-in rules reach one cell
    assert not fired[2].any() and not fired[5].any() and not fired[7].any() and not fired[8].any()
    assert np.array_equal(TA.scores(best, surv, "noisy_or")[0], np.array([0, 0, 0.625, 0, 0], np.float32))
    # the rules the issue names, alone: r0[any] ^ r1[now] -> r1 and r0^-1[future] ^ r0[any] -> r1
    one = lambda i: TA.apply_dense(*args[:4], TA.HAND_HEAD[i:i + 1], TA.HAND_BODY[i:i + 1], TA.HAND_DIR[i:i + 1], TA.HAND_WEIGHT[i:i + 1],
                                   *args[8:])[3]
    assert np.argwhere(one(1)).tolist() == [[0, 2], [1, 2]]
    assert np.argwhere(one(2)).tolist() == [[3, 1], [4, 1]]


def test_the_two_references_agree_and_ranges_change_nothing():
    n_ent, n_rela, n_time, quads, rng = _small()
    B = 90
    subs, rels, times = rng.integers(0, n_ent, B), rng.integers(0, n_rela, B), rng.integers(0, n_time, B)
    rels[:70] = rng.choice([0, 4], 70)                                  # 70 queries of two relations: more than a 64-bit word
    subs[1], rels[1], times[1] = subs[0], rels[0], times[0]             # a query stated twice
    some2 = False
    for L in (1, 2, 3):
        head, body, direc, weight = _rules(rng, 24, L, n_rela, [0, 4, 5])
        args = (n_ent, n_rela, n_time, quads)
        dense = TA.apply_dense(*args, head, body, direc, weight, subs, rels, times)
        cells = TA.apply_cells(*args, head, body, direc, weight, subs, rels, times)
        assert A.same(A.cells_to_dense(cells, B, n_ent), dense)
        assert (dense[3] > 0).sum() > 50 and set(direc.reshape(-1).tolist()) == {0, 1, 2, 3}
        assert np.array_equal(dense[0][0], dense[0][1]) and np.array_equal(dense[3][0], dense[3][1])
        some2 |= bool((dense[3] >= 2).any())
        # rules cut into ranges, carried through state and rule_base
        state_d, state_c = None, None
        for r0, r1 in ((0, 5), (5, 6), (6, 24)):
            part = (head[r0:r1], body[r0:r1], direc[r0:r1], weight[r0:r1], subs, rels, times)
            state_d = TA.apply_dense(*args, *part, state=state_d, rule_base=r0)
            state_c = TA.apply_cells(*args, *part, state=state_c, rule_base=r0)
        assert A.same(state_d, dense) and state_c == cells
    assert some2


def _graph(n_ent=5, n_rela_rows=7, n_time=3):
    return types.SimpleNamespace(n_ent=n_ent, n_rela_rows=n_rela_rows, n_time=n_time)


def test_check_trule_apply():
    g = _graph()
    good = dict(head=TA.HAND_HEAD, body=TA.HAND_BODY, direction=TA.HAND_DIR, weight=TA.HAND_WEIGHT, subs=TA.HAND_SUBS,
                rels=TA.HAND_RELS, times=TA.HAND_TIMES)
    out = check_trule_apply(g, **good)
    assert [a.dtype for a in out] == [np.int32, np.int32, np.int32, np.float32, np.int32, np.int32, np.int32]
    assert all(a.flags.c_contiguous for a in out) and np.array_equal(out[2], TA.HAND_DIR) and np.array_equal(out[6], TA.HAND_TIMES)
    as_t = {k: torch.as_tensor(v) for k, v in good.items()}
    assert all(np.array_equal(a, b) for a, b in zip(check_trule_apply(g, **as_t), out))
    bad = lambda **kw: check_trule_apply(g, **dict(good, **kw))
    for kw, match in ((dict(head=TA.HAND_HEAD[::-1].copy()), "trule_apply: head must be non-decreasing"),
                      (dict(body=TA.HAND_BODY + 1), r"trule_apply: relation id out of range 0\.\.6"),
                      (dict(head=TA.HAND_HEAD - 1), r"trule_apply: relation id out of range 0\.\.6"),
                      (dict(direction=TA.HAND_DIR + 1), r"trule_apply: direction out of range 0\.\.3"),
                      (dict(direction=TA.HAND_DIR[:, :1]), "trule_apply: head must be"),
                      (dict(body=TA.HAND_BODY.astype(np.float32)), "trule_apply: body must be int32 or int64"),
                      (dict(weight=np.array([0.5, 0.25, 0.0, 0.5], np.float32)), r"trule_apply: weights must be finite and in \(0, 1\]"),
                      (dict(weight=np.array([0.5, 1.25, 0.5, 0.5], np.float32)), r"trule_apply: weights must be finite and in \(0, 1\]"),
                      (dict(weight=np.array([0.5, np.nan, 0.5, 0.5], np.float32)), r"trule_apply: weights must be finite and in \(0, 1\]"),
                      (dict(weight=np.array([1, 1, 1, 1])), "trule_apply: weight must be a float array"),
                      (dict(weight=TA.HAND_WEIGHT[:3]), "trule_apply: weight must be a float array"),
                      (dict(subs=TA.HAND_SUBS + 2), r"trule_apply: subject id out of range 0\.\.4"),
                      (dict(rels=TA.HAND_RELS + 6), r"trule_apply: query relation id out of range 0\.\.6"),
                      (dict(times=TA.HAND_TIMES + 1), r"trule_apply: query time id out of range 0\.\.2"),
                      (dict(times=TA.HAND_TIMES - 1), r"trule_apply: query time id out of range 0\.\.2"),
                      (dict(times=TA.HAND_TIMES[:-1]), "trule_apply: need one relation and one time per subject"),
                      (dict(rels=TA.HAND_RELS[:-1]), "trule_apply: need one relation and one time per subject")):
        with pytest.raises(ValueError, match=match):
            bad(**kw)
    with pytest.raises(ValueError, match="trule_apply: the body length 33 is not in"):
        bad(body=np.zeros((4, 33), np.int64), direction=np.zeros((4, 33), np.int64))
    with pytest.raises(ValueError, match="trule_apply: static graph"):
        check_trule_apply(_graph(n_time=0), **good)
    with pytest.raises(ValueError, match="trule_apply: scratch_bytes must be a non-negative integer"):
        trule_apply(g, scratch_bytes=-1, **good)
    # no rule, no query: validated all the same
    empty = check_trule_apply(g, TA.HAND_HEAD[:0], TA.HAND_BODY[:0], TA.HAND_DIR[:0], TA.HAND_WEIGHT[:0], TA.HAND_SUBS[:0],
                                     TA.HAND_RELS[:0], TA.HAND_TIMES[:0])
    assert empty[0].shape == (0,) and empty[1].shape == (0, 2) and empty[4].shape == (0,)


def test_rule_apply_still_refuses_a_temporal_graph():
    from red_gnn_amd import engine
    with pytest.raises(ValueError, match="^rule_apply: temporal graph.*trule_apply"):
        engine.rule_apply(_graph(), np.array([0]), np.array([[0, 1]]), np.array([0.5], np.float32), np.array([0]), np.array([0]))


def _quality():
    from red_gnn_amd.explain import TemporalRuleQuality, TemporalRuleTable
    n_rel = 6                                                # the model's n_rel: 6 is the identity
    head = torch.tensor([0, 0, 1, 1, 2])
    body = torch.tensor([[6, 0], [3, 4], [1, 6], [2, 2], [0, 1]])
    direc = torch.tensor([[3, 1], [0, 2], [0, 3], [1, 1], [3, 3]])      # row 0: id ^ r0[now] -> r0 is trivial; row 2 (r1[past]) is not
    one = torch.ones(5, dtype=torch.int64)
    table = TemporalRuleTable(head, body, direc, one, one.clone(), n_rel)
    return TemporalRuleQuality(table, body_pairs=torch.tensor([4, 10, 8, 0, 3]), hits=torch.tensor([4, 5, 1, 0, 3]),
                               pca_body_pairs=torch.tensor([4, 8, 2, 0, 3]), head_pairs=torch.tensor([4, 9, 9, 9, 5]), n_anchors=7)


def test_rule_weights_takes_a_temporal_quality():
    from red_gnn_amd import explain
    q = _quality()
    assert q.trivial().tolist() == [True, False, False, False, False]
    rows, w = explain.rule_weights(q)
    assert rows.dtype == np.int64 and w.dtype == np.float32
    assert rows.tolist() == [1, 2, 4] and w.tolist() == [0.5, 0.125, 1.0]
    rows, w = explain.rule_weights(q, drop_trivial=False)
    assert rows.tolist() == [0, 1, 2, 4] and w.tolist() == [1.0, 0.5, 0.125, 1.0]
    rows, w = explain.rule_weights(q, by="pca_confidence", laplace=2.0, min_hits=3)
    assert rows.tolist() == [1, 4] and np.array_equal(w, np.array([5 / 10.0, 3 / 5.0]).astype(np.float32))
    with pytest.raises(ValueError, match="rule_scores: by must be"):
        explain.rule_weights(q, by="hits")
    with pytest.raises(ValueError, match="rule_scores: laplace must be"):
        explain.rule_weights(q, laplace=-1.0)
    with pytest.raises(ValueError, match="rule_scores: quality must be an explain.RuleQuality"):
        explain.rule_weights(q.table)
    # the static driver keeps rejecting the temporal table, and the temporal one the static table
    model = types.SimpleNamespace(n_rel=6)
    with pytest.raises(ValueError, match=r"rule_scores: quality must be an explain.RuleQuality \(got TemporalRuleQuality\)"):
        explain.rule_scores(model, q, np.array([0]), np.array([0]))
    static = explain.RuleQuality(explain.RuleTable(q.table.head, q.table.body, q.table.support, q.table.fixed, 6), q.body_pairs, q.hits,
                                 q.pca_body_pairs, q.head_pairs, 7)
    batch = {"head": np.array([0]), "relation": np.array([0]), "time": np.array([0])}
    with pytest.raises(ValueError, match=r"rule_scores: quality must be an explain.TemporalRuleQuality \(got RuleQuality\)"):
        explain.temporal_rule_scores(model, static, batch)
    with pytest.raises(ValueError, match="rule_scores: the table has n_rel=6, the model n_rel=5"):
        explain.temporal_rule_scores(types.SimpleNamespace(n_rel=5), q, batch)
    with pytest.raises(ValueError, match="rule_evaluate: give exactly one of quality"):
        explain.temporal_rule_evaluate(model, np.zeros((1, 4), np.int64))
    with pytest.raises(ValueError, match="rule_evaluate: give exactly one of quality"):
        explain.temporal_rule_evaluate(model, np.zeros((1, 4), np.int64), quality=q, mine=np.zeros((1, 4), np.int64))


def test_filter_lists():
    from red_gnn_amd.explain import temporal_filter_lists
    known = (np.array([3, 7, 9]), np.array([0, 2, 3, 6]), np.array([1, 4, 2, 0, 5, 8], np.int32))
    ptr, idx = temporal_filter_lists(np.array([7, 9, 4, 3]), np.array([2, 6, 1, 9]), known)
    assert ptr.tolist() == [0, 1, 5, 6, 9] and idx.tolist() == [2, 0, 5, 6, 8, 1, 1, 4, 9]
    assert ptr.dtype == np.int32 and idx.dtype == np.int32
    ptr, idx = temporal_filter_lists(np.array([7, 9]), np.array([2, 6]), None)
    assert ptr.tolist() == [0, 1, 2] and idx.tolist() == [2, 6]


def test_symbol_and_entry_checks():
    from red_gnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redgnn.h")).read(), flags=re.S)
    assert re.search(r"\brg_trule_apply\s*\(", text) and "rg_trule_apply" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "rg_trule_apply") and L.rg_version() == 12
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: NULL graph"):
        _lib.check(L.rg_trule_apply(None, None, None, None, None, None, 1, 2, 0, None, None, None, 1, None, 3, None, 3, None, None,
                                    None, None, None))
