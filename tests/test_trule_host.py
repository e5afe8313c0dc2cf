"""The host side of the temporal rules (no GPU): explain.TemporalRuleTable / temporal_rules_from_paths on a hand-made temporal r-digraph,
explain.TemporalRuleQuality's ratios and ordering, the two new C symbols in the header and in _lib.SYMBOLS, and engine.trule_ground's
validation, which runs before anything touches a device."""
import os
import re
import types

import numpy as np
import pytest
import torch

from red_gnn_amd.explain import (PathSet, RDigraph, RuleQuality, RuleTable, TemporalRuleQuality, TemporalRuleTable,
                                 temporal_rules_from_paths)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REL = 6                    # the model's n_rel: relation ids 0..5 as the quadruples hold them, 6 the identity


def _digraph():
    # query times: row 0 at 5, row 1 at 3, row 2 (no edge) at 0.  Edge times against them give the directions in the comments.
    # row 0: 0 -r0-> 1 (t 2: past)  0 -r1-> 2 (t 5: now)  0 -r0-> 2 (t 9: future)  1 -r4-> 9 (t 5: now)  2 -r4-> 9 (t 7: future)
    # row 1: 5 -id-> 5 (t 11, the sentinel: "future" here, written as any)  5 -r2-> 7 (t 1: past)
    edges = torch.tensor([[0, 1, 0, 0, 1], [0, 1, 0, 1, 2], [0, 1, 0, 0, 2], [0, 2, 1, 4, 9], [0, 2, 2, 4, 9],
                          [1, 1, 5, 6, 5], [1, 2, 5, 2, 7]], dtype=torch.int32)
    alpha = torch.tensor([0.5, 0.25, 0.75, 1.0, 0.5, 0.125, 0.5], dtype=torch.float32)
    return RDigraph(edges=edges, alpha=alpha, offsets=torch.tensor([0, 5, 7, 7]), reached=torch.tensor([True, True, False]),
                    score=torch.zeros(3), n_hops=2, time=torch.tensor([2, 5, 9, 5, 7, 11, 1], dtype=torch.int32),
                    q_time=torch.tensor([5, 3, 0], dtype=torch.int32))


def _paths():
    # row 0: (e0, e3) = r0[past] r4[now]; (e2, e4) = r0[future] r4[future]; (e1, e4) = r1[now] r4[future];  row 1: (e5, e6)
    edge = torch.tensor([[[0, 3], [2, 4], [1, 4]], [[5, 6], [-1, -1], [-1, -1]], [[-1, -1]] * 3])
    product = torch.tensor([[0.5, 0.375, 0.125], [0.0625, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    return PathSet(edge=edge, product=product, count=torch.tensor([3, 1, 0], dtype=torch.int32), digraph=_digraph())


def _same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "direction", "support", "fixed")) and a.n_rel == b.n_rel


def test_temporal_rules_from_paths():
    assert _digraph().direction().tolist() == [0, 1, 2, 1, 2, 2, 0]
    t = temporal_rules_from_paths(_paths(), [1, 2, 0], N_REL)
    assert isinstance(t, TemporalRuleTable)
    # sorted by (head, r_1, d_1, r_2, d_2); the identity step of row 1 is "any" although its edge lies in the query's future
    assert t.head.tolist() == [1, 1, 1, 2]
    assert t.body.tolist() == [[0, 4], [0, 4], [1, 4], [6, 2]]
    assert t.direction.tolist() == [[0, 1], [2, 2], [1, 2], [3, 0]]
    assert t.support.tolist() == [1, 1, 1, 1]
    assert t.fixed.tolist() == [int(0.5 * 2 ** 32), int(0.375 * 2 ** 32), int(0.125 * 2 ** 32), int(0.0625 * 2 ** 32)]
    assert t.product_sum().tolist() == [0.5, 0.375, 0.125, 0.0625] and t.mean().tolist() == [0.5, 0.375, 0.125, 0.0625]
    assert t.key().tolist()[0] == [1, 0, 0, 4, 1] and t.key().tolist() == sorted(t.key().tolist())
    # equal keys merge: the same two rows once more, under the same query relation
    ps = _paths()
    twice = PathSet(torch.cat([ps.edge[:1], ps.edge[:1]]), torch.cat([ps.product[:1], ps.product[:1]]),
                    torch.cat([ps.count[:1], ps.count[:1]]), ps.digraph)
    m = temporal_rules_from_paths(twice, [1, 1], N_REL)
    assert m.head.tolist() == [1, 1, 1] and m.support.tolist() == [2, 2, 2] and m.fixed.tolist() == [2 * x for x in t.fixed.tolist()[:3]]
    # each path is rounded once, to the nearest unit of 2^-32 (halves up), as rules_from_paths rounds
    ps.product[0] = torch.tensor([1.5 * 2.0 ** -32, 2.0 ** -33, 0.49 * 2.0 ** -32], dtype=torch.float64)
    assert temporal_rules_from_paths(ps, [1, 2, 0], N_REL).fixed.tolist() == [2, 1, 0, int(0.0625 * 2 ** 32)]
    with pytest.raises(ValueError):
        temporal_rules_from_paths(_paths(), [1, 2], N_REL)
    with pytest.raises(ValueError):
        temporal_rules_from_paths(_paths(), [1, 2, 7], N_REL)
    static = _paths()
    static.digraph.time = None
    with pytest.raises(ValueError, match="static r-digraph"):
        temporal_rules_from_paths(static, [1, 2, 0], N_REL)
    none = temporal_rules_from_paths(PathSet(ps.edge[2:], ps.product[2:], ps.count[2:], ps.digraph), [0], N_REL)
    assert none.head.numel() == 0 and none.body.shape == (0, 2) and none.direction.shape == (0, 2) and none.format() == []


def test_format_top_and_cpu():
    t = temporal_rules_from_paths(_paths(), [1, 2, 0], N_REL)
    assert t.format() == ["r0[past](x,z1) ^ r4[now](z1,y) -> r1(x,y)", "r0[future](x,z1) ^ r4[future](z1,y) -> r1(x,y)",
                          "r1[now](x,z1) ^ r4[future](z1,y) -> r1(x,y)", "r2[past](x,y) -> r2(x,y)"]
    names = ["born", "lives", "works", "born_inv", "lives_inv", "works_inv"]
    assert t.format(names)[3] == "works[past](x,y) -> works(x,y)"
    only_pad = TemporalRuleTable(torch.tensor([1, 0]), torch.tensor([[6, 6], [3, 6]]), torch.tensor([[3, 3], [3, 3]]),
                                 torch.tensor([1, 1]), torch.tensor([5, 5]), N_REL)
    assert only_pad.format() == ["x=y -> r1(x,y)", "r3(x,y) -> r0(x,y)"]             # no tag for "any"
    t.support[:] = torch.tensor([2, 5, 5, 1])
    top = t.top(1, 2)
    assert top.body.tolist() == [[0, 4], [1, 4]] and top.direction.tolist() == [[2, 2], [1, 2]] and top.support.tolist() == [5, 5]
    assert t.top(2, 5).head.tolist() == [2] and t.top(4, 1).head.numel() == 0
    with pytest.raises(ValueError):
        t.top(1, 0)
    assert _same(t.cpu(), t)


def test_add_is_the_table_of_the_concatenation():
    rng = np.random.default_rng(0)
    rd = _digraph()
    B, k, E = 40, 3, rd.edges.shape[0]
    rd.q_time = torch.from_numpy(rng.integers(0, 12, B).astype(np.int32))
    rd.edges[:, 0] = torch.from_numpy(rng.integers(0, B, E).astype(np.int32))       # directions are read per edge, whatever the row
    edge = torch.from_numpy(rng.integers(0, E, (B, k, 2)))
    count = torch.from_numpy(rng.integers(0, k + 1, B).astype(np.int32))
    edge[torch.arange(k)[None, :] >= count[:, None]] = -1
    product = torch.from_numpy(rng.uniform(0, 1, (B, k)))
    q = rng.integers(0, N_REL, B)
    whole = temporal_rules_from_paths(PathSet(edge, product, count, rd), q, N_REL)
    parts = None
    for lo, hi in ((0, 7), (7, 8), (8, 30), (30, 40)):
        p = temporal_rules_from_paths(PathSet(edge[lo:hi], product[lo:hi], count[lo:hi], rd), q[lo:hi], N_REL)
        parts = p if parts is None else parts + p
    assert _same(whole, parts) and whole.support.sum() == count.sum()
    key = whole.key().tolist()
    assert key == sorted(key) and len({tuple(x) for x in key}) == len(key)
    assert ((whole.direction == 3) == (whole.body == N_REL)).all()
    empty = temporal_rules_from_paths(PathSet(edge[:0], product[:0], count[:0], rd), q[:0], N_REL)
    assert _same(whole + empty, whole) and _same(empty + whole, whole)
    with pytest.raises(ValueError):
        whole + TemporalRuleTable(whole.head, whole.body, whole.direction, whole.support, whole.fixed, N_REL + 2)
    with pytest.raises(TypeError):
        whole + RuleTable(whole.head, whole.body, whole.support, whole.fixed, N_REL)


def _quality():
    head = torch.tensor([0, 0, 0, 0, 1, 0])
    body = torch.tensor([[6, 0], [0, 6], [6, 0], [2, 3], [6, 1], [1, 3]])
    direc = torch.tensor([[3, 1], [1, 3], [3, 0], [0, 2], [3, 1], [3, 3]])
    one = torch.ones(6, dtype=torch.int64)
    table = TemporalRuleTable(head, body, direc, one, one.clone(), N_REL)
    t = lambda *x: torch.tensor(x, dtype=torch.int64)
    return TemporalRuleQuality(table, body_pairs=t(8, 8, 10, 4, 3, 0), hits=t(8, 8, 5, 2, 3, 0), pca_body_pairs=t(8, 8, 5, 4, 3, 0),
                               head_pairs=t(8, 8, 8, 8, 3, 8), n_anchors=7)


def test_temporal_rule_quality():
    q = _quality()
    assert q.confidence().tolist() == [1.0, 1.0, 0.5, 0.5, 1.0, 0.0]
    assert q.pca_confidence().tolist() == [1.0, 1.0, 1.0, 0.5, 1.0, 0.0]
    assert q.head_coverage().tolist() == [1.0, 1.0, 0.625, 0.25, 1.0, 0.0]
    # trivial: exactly one non-identity step, the head relation, taken now; the same step in the past is a real rule
    assert q.trivial().tolist() == [True, True, False, False, True, False]
    assert q.top(0, 5).tolist() == [2, 3]                       # both have confidence 0.5: the larger hits (5 against 2) first
    assert q.top(0, 5, by="hits").tolist() == [2, 3]
    assert q.top(0, 5, by="pca_confidence").tolist() == [2, 3]
    assert q.top(0, 1, drop_trivial=False).tolist() == [1]      # rows 0 and 1 tie on score and hits: the smaller (r, d) key wins
    assert q.top(0, 9, min_hits=0).tolist() == [2, 3, 5] and q.top(1, 3).numel() == 0
    with pytest.raises(ValueError):
        q.top(0, 3, by="support")
    lines = q.format()
    assert lines[2] == "r0[past](x,y) -> r0(x,y)  5/10 conf=0.5000 pca=1.0000" and len(lines) == 6
    c = q.cpu()
    assert isinstance(c, TemporalRuleQuality) and c.n_anchors == 7 and torch.equal(c.hits, q.hits)
    # the two quality classes share the ratio and ordering code
    assert RuleQuality.confidence is TemporalRuleQuality.confidence and RuleQuality.top is TemporalRuleQuality.top


def test_header_and_binding_carry_the_symbols():
    from red_gnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redgnn.h")).read(), flags=re.S)
    for name in ("rg_trule_ground_scratch_bytes", "rg_trule_ground"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    L = _lib.lib()
    for args in ((300, 5, 33), (1, 1, 1), (0, 1, 1), (5, 0, 1), (5, 1, 0), (5, 65536, 1), (2 ** 31 - 1, 65535, 2 ** 31 - 1)):
        assert L.rg_trule_ground_scratch_bytes(*args) == L.rg_rule_ground_scratch_bytes(*args), args
    assert L.rg_trule_ground_scratch_bytes(300, 5, 33) > 0 and L.rg_trule_ground_scratch_bytes(5, 65536, 1) == 0
    with pytest.raises(_lib.NativeError, match="rg_trule_ground: NULL graph"):
        _lib.check(L.rg_trule_ground(None, None, None, None, 1, 1, None, None, 1, None, None, None))


def test_engine_validates_on_the_host():
    from red_gnn_amd import engine
    g = types.SimpleNamespace(n_ent=5, n_rela_rows=7, n_time=3)            # no handle, no device: validation never asks for them
    head, body, direc = np.array([0, 1]), np.array([[0, 6], [2, 3]]), np.array([[0, 3], [1, 2]])
    anchors = np.array([[0, 0], [4, 2]])
    cases = [
        ("static graph", dict(graph=types.SimpleNamespace(n_ent=5, n_rela_rows=7, n_time=0))),
        ("head must be", dict(body=body[:1])),
        ("head must be", dict(direction=direc[:, :1])),
        ("must be int32 or int64", dict(direction=direc.astype(np.float64))),
        ("must be int32 or int64", dict(anchors=anchors.astype(np.float32))),
        ("body length 33", dict(body=np.zeros((2, 33), np.int64), direction=np.zeros((2, 33), np.int64))),
        (r"relation id out of range 0\.\.6", dict(body=np.array([[0, 7], [2, 3]]))),
        (r"relation id out of range 0\.\.6", dict(head=np.array([0, -1]))),
        (r"direction out of range 0\.\.3", dict(direction=np.array([[0, 4], [1, 2]]))),
        (r"direction out of range 0\.\.3", dict(direction=np.array([[0, -1], [1, 2]]))),
        (r"anchors must be \[S, 2\]", dict(anchors=np.array([0, 1, 2]))),
        ("anchor out of range", dict(anchors=np.array([[5, 0]]))),
        ("anchor out of range", dict(anchors=np.array([[0, 3]]))),
        ("anchor out of range", dict(anchors=np.array([[-1, 0]]))),
        ("duplicate anchors", dict(anchors=np.array([[1, 2], [0, 0], [1, 2]]))),
        ("scratch_bytes must be", dict(scratch_bytes=-1)),
        ("scratch_bytes must be", dict(scratch_bytes=1.5)),
        ("scratch_bytes must be", dict(scratch_bytes=True)),
    ]
    for match, change in cases:
        kw = dict(graph=g, head=head, body=body, direction=direc, anchors=anchors)
        kw.update(change)
        with pytest.raises(ValueError, match="trule_ground: .*" + match):
            engine.trule_ground(**kw)
    # what validation hands on: int32 arrays and the anchors sorted by (time, entity)
    h, b, d, a = engine.check_trules(g, head, torch.as_tensor(body), direc, np.array([[4, 2], [1, 0], [0, 2], [3, 0]]))
    assert h.dtype == b.dtype == d.dtype == np.int32 and a.tolist() == [[1, 0], [3, 0], [0, 2], [4, 2]]
