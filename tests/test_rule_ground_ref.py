"""Rule quality without a device: the numpy references of tests/rule_ground_ref.py on a graph written out by hand, with the counts
typed in; the arithmetic of explain.RuleQuality; and the host validation and chunking of engine.rule_ground."""
import types

import numpy as np
import pytest
import torch

from tests import rule_ground_ref as R


@pytest.mark.parametrize("fn", [R.counts_dense, R.counts])
def test_hand_graph_counts(fn):
    rows = R.hand_rows()
    assert len(rows) == 2 * len(R.HAND_TRIPLES) + R.HAND_N_ENT
    assert np.array_equal(fn(R.HAND_N_ENT, 5, rows, R.HAND_HEAD, R.HAND_BODY), R.HAND_ALL)
    assert np.array_equal(fn(R.HAND_N_ENT, 5, rows, R.HAND_HEAD, R.HAND_BODY, R.HAND_SOURCES), R.HAND_SUB)
    assert fn(R.HAND_N_ENT, 5, rows, R.HAND_HEAD[:0], R.HAND_BODY[:0]).shape == (0, 4)


def test_rows_from_export_is_rows_from_triples():
    rows = R.hand_rows()
    order = np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))
    rows = rows[order]
    out_ptr = np.searchsorted(rows[:, 0], np.arange(R.HAND_N_ENT + 1))
    again = R.rows_from_export(out_ptr, rows[:, 1:])
    assert np.array_equal(again, rows)


def test_expansion_is_the_dense_chain_on_random_graphs():
    rng = np.random.default_rng(2)
    for n_ent, n_rel, n_trip, L in ((40, 3, 90, 1), (40, 3, 90, 3), (67, 2, 60, 4)):
        trip = np.stack([rng.integers(0, n_ent, n_trip), rng.integers(0, n_rel, n_trip), rng.integers(0, n_ent, n_trip)], 1)
        rows = R.rows_from_triples(n_ent, n_rel, np.concatenate([trip, trip[:7]], 0))
        n_rela = 2 * n_rel + 1
        head, body = rng.integers(0, n_rela, 30), np.sort(rng.integers(0, n_rela, (30, L)), 0)      # shared prefixes
        for sources in (None, rng.permutation(n_ent)[:33], rng.permutation(n_ent)[:1]):
            a, b = R.counts_dense(n_ent, n_rela, rows, head, body, sources), R.counts(n_ent, n_rela, rows, head, body, sources)
            assert np.array_equal(a, b)
            assert (a[:, 1] <= a[:, 2]).all() and (a[:, 2] <= a[:, 0]).all() and (a[:, 1] <= a[:, 3]).all()


def test_sparse_chain_is_the_dense_chain():
    rows = R.hand_rows()
    assert np.array_equal(R.counts_sparse(R.HAND_N_ENT, 5, rows, R.HAND_HEAD, R.HAND_BODY), R.HAND_ALL)
    n_ent, n_rel, n_rela, trip = R.wide_graph(67)
    rows = R.rows_from_triples(n_ent, n_rel, trip)
    head, body = R.wide_rules(n_rela)
    a = R.counts_dense(n_ent, n_rela, rows, head, body)
    assert np.array_equal(a, R.counts_sparse(n_ent, n_rela, rows, head, body))
    assert ((a[:, 1] > 0) & (a[:, 1] < a[:, 0])).any() and (a[:, 0] == 0).any() and (a[-1, 1] > 0) and (a[-1, 1] < a[-1, 0])


# ---- explain.RuleQuality ---------------------------------------------------------------------------------------------

def _quality():
    from red_gnn_amd.explain import RuleQuality, RuleTable
    t = lambda x: torch.tensor(x, dtype=torch.int64)
    # n_rel = 2, identity = 4.  Rows sorted by (head, body), as RuleTable keeps them.
    head = t([0, 0, 0, 0, 0, 0, 1, 1])
    body = t([[0, 4], [1, 2], [1, 3], [2, 3], [3, 1], [4, 0], [0, 1], [4, 4]])
    table = RuleTable(head, body, t([1] * 8), t([0] * 8), 2)
    #               trivial  c=.5   c=.5    c=.5   c=1 h=1  trivial  head 1  nothing
    body_pairs = t([3,       4,     8,      8,     1,       3,       2,      0])
    hits = t([3,             2,     4,      4,     1,       3,       1,      0])
    pca = t([3,              2,     5,      4,     1,       3,       2,      0])
    head_pairs = t([5,       5,     5,      5,     5,       5,       0,      0])
    return RuleQuality(table, body_pairs, hits, pca, head_pairs, 5)


def test_rule_quality_ratios_and_zero_denominators():
    q = _quality()
    assert q.confidence().dtype == torch.float64
    assert q.confidence().tolist() == [1.0, 0.5, 0.5, 0.5, 1.0, 1.0, 0.5, 0.0]
    assert q.pca_confidence().tolist() == [1.0, 1.0, 0.8, 1.0, 1.0, 1.0, 0.5, 0.0]
    assert q.head_coverage().tolist() == [3 / 5, 2 / 5, 4 / 5, 4 / 5, 1 / 5, 3 / 5, 0.0, 0.0]
    assert q.trivial().tolist() == [True, False, False, False, False, True, False, False]
    c = q.cpu()
    assert c.n_sources == 5 and torch.equal(c.hits, q.hits) and torch.equal(c.table.body, q.table.body)


def test_rule_quality_top_order_and_ties():
    q = _quality()
    # confidence: row 4 (1.0) first; rows 2 and 3 (0.5, hits 4) before row 1 (0.5, hits 2); 2 before 3 by the smaller body
    assert q.top(0, 10).tolist() == [4, 2, 3, 1]
    assert q.top(0, 2).tolist() == [4, 2]
    assert q.top(0, 10, drop_trivial=False).tolist() == [0, 5, 4, 2, 3, 1]       # hits 3 before hits 1 at confidence 1
    assert q.top(0, 10, by="hits").tolist() == [2, 3, 1, 4]
    assert q.top(0, 10, by="pca_confidence").tolist() == [3, 1, 4, 2]           # 1.0 three times: hits 4, 2, 1; then 0.8
    assert q.top(0, 10, min_hits=3).tolist() == [2, 3]
    assert q.top(1, 10).tolist() == [6] and q.top(1, 10, min_hits=0).tolist() == [6, 7]
    assert q.top(3, 10).tolist() == [] and q.top(3, 10).dtype == torch.int64
    for bad in (dict(n=0), dict(n=True), dict(n=2, by="support")):
        with pytest.raises(ValueError, match="top:"):
            q.top(0, **bad)


def test_rule_quality_format():
    q = _quality()
    lines = q.format()
    assert lines[1] == "r1(x,z1) ^ r0^-1(z1,y) -> r0(x,y)  2/4 conf=0.5000 pca=1.0000"
    assert lines[0] == "r0(x,y) -> r0(x,y)  3/3 conf=1.0000 pca=1.0000"
    assert lines[7] == "x=y -> r1(x,y)  0/0 conf=0.0000 pca=0.0000"
    assert q.format(["parent", "sibling"])[2] == "sibling(x,z1) ^ sibling^-1(z1,y) -> parent(x,y)  4/8 conf=0.5000 pca=0.8000"
    assert [l.split("  ")[0] for l in lines] == q.table.format()


# ---- host validation and chunking of engine.rule_ground --------------------------------------------------------------

def _graph(**kw):
    return types.SimpleNamespace(**dict(dict(n_ent=5, n_rel=2, n_time=0, device="cuda", handle=None), **kw))


@pytest.mark.parametrize("kw, text", [
    (dict(head=np.array([0.0]), body=np.array([[0, 1]])), "head must be int32 or int64"),
    (dict(head=np.array([0]), body=np.array([[0.5, 1]])), "body must be int32 or int64"),
    (dict(head=np.array([0, 1]), body=np.array([[0, 1]])), r"head must be \[R\] and body \[R, L\]"),
    (dict(head=np.array([0]), body=np.array([0, 1])), r"head must be \[R\] and body \[R, L\]"),
    (dict(head=np.array([0]), body=np.zeros((1, 0), np.int64)), "body length 0 is not in 1..32"),
    (dict(head=np.array([0]), body=np.zeros((1, 33), np.int64)), "body length 33 is not in 1..32"),
    (dict(head=np.array([5]), body=np.array([[0, 1]])), r"relation id out of range 0\.\.4"),
    (dict(head=np.array([0]), body=np.array([[0, -1]])), r"relation id out of range 0\.\.4"),
    (dict(head=np.array([0]), body=np.array([[0, 1]]), sources=np.array([0, 5])), r"source id out of range 0\.\.4"),
    (dict(head=np.array([0]), body=np.array([[0, 1]]), sources=np.array([-1])), r"source id out of range 0\.\.4"),
    (dict(head=np.array([0]), body=np.array([[0, 1]]), sources=np.array([2, 1, 2])), "duplicate sources"),
    (dict(head=np.array([0]), body=np.array([[0, 1]]), sources=np.array([[0, 1]])), r"sources must be \[S\]"),
    (dict(head=np.array([0]), body=np.array([[0, 1]]), sources=np.array([0.0])), "sources must be int32 or int64"),
    (dict(head=np.array([0]), body=np.array([[0, 1]]), scratch_bytes=-1), "scratch_bytes must be a non-negative integer"),
])
def test_rule_ground_value_errors(kw, text):
    from red_gnn_amd import engine
    with pytest.raises(ValueError, match="rule_ground: .*" + text):
        engine.rule_ground(_graph(), **kw)


def test_rule_ground_refuses_a_temporal_graph_and_another_n_rel():
    from red_gnn_amd import engine, explain
    with pytest.raises(ValueError, match="rule_ground: temporal graph"):
        engine.rule_ground(_graph(n_rel=0, n_time=7), np.array([0]), np.array([[0, 1]]))
    table = _quality().table
    with pytest.raises(ValueError, match="rule_quality: the table has n_rel=2, the model n_rel=3"):
        explain.rule_quality(types.SimpleNamespace(n_rel=3), table)
    with pytest.raises(ValueError, match="rule_quality: table must be an explain.RuleTable"):
        explain.rule_quality(types.SimpleNamespace(n_rel=2), (table.head, table.body))


def test_check_rules_accepts_tensors_and_fills_sources():
    from red_gnn_amd import engine
    h, b, s = engine.check_rules(5, 2, torch.tensor([4, 0]), torch.tensor([[0, 4], [3, 2]], dtype=torch.int32))
    assert h.dtype == b.dtype == s.dtype == np.int32 and b.flags.c_contiguous
    assert h.tolist() == [4, 0] and b.tolist() == [[0, 4], [3, 2]] and s.tolist() == [0, 1, 2, 3, 4]
    assert engine.check_rules(5, 2, h[:0], b[:0], np.array([4, 2]))[2].tolist() == [4, 2]


def test_rule_chunking_and_scratch_bytes():
    from red_gnn_amd import engine
    need = engine.rule_ground_scratch_bytes
    assert need(300, 1, 32) >= 3 * 300 * 4 + 4 and need(300, 1, 33) >= 3 * 300 * 8 + 8
    assert need(300, 1, 32) == need(300, 1, 1) < need(300, 1, 33) == need(300, 1, 64) < need(300, 2, 64)
    assert need(0, 1, 1) == 0 and need(1, 0, 1) == 0 and need(1, 1, 0) == 0 and need(1, 65536, 1) == 0
    assert need(1 << 30, 65535, 1 << 30) == 0                                   # beyond 2^40 words per bitmap
    assert (3 << 31) < need(1 << 20, 1, 1 << 16) < (1 << 62)                    # 2^31 words per bitmap: sized in 64 bits
    assert engine.rule_chunking(300, 64, 300, 1 << 30) == (64, 320)             # everything in one chunk
    assert engine.rule_chunking(300, 64, 300, need(300, 1, 32)) == (1, 32)      # the smallest chunk
    assert engine.rule_chunking(300, 64, 300, 0) == (1, 32)                     # ... which a budget below it still gets
    assert engine.rule_chunking(300, 64, 300, need(300, 1, 320)) == (1, 320)
    assert need(300, 1, 320) < need(300, 5, 96) < need(300, 2, 320)
    assert engine.rule_chunking(300, 64, 300, need(300, 5, 96)) == (1, 320)     # all sources of one rule come before more rules
    assert engine.rule_chunking(300, 64, 300, need(300, 1, 320) - 1) == (1, 288)
    n_r, s_c = engine.rule_chunking(300, 64, 65, need(300, 7, 96))
    assert (n_r, s_c) == (7, 96)
