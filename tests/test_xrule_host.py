"""The host side of the extrapolation rules (no GPU): explain.LagRuleTable / lag_rules_from_paths on a hand-made extrapolation
r-digraph, explain.LagRuleQuality's ratios and ordering, the new C symbol in the header and in _lib.SYMBOLS, and engine.xrule_ground's
validation, which runs before anything touches a device."""
import os
import re
import types

import numpy as np
import pytest
import torch

from red_gnn_amd import profile
from red_gnn_amd.explain import (LagRuleQuality, LagRuleTable, PathSet, RDigraph, RuleQuality, RuleTable, TemporalRuleTable,
                                 lag_rules_from_paths)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REL = 6                    # the identity's id: relation ids 0..5 as the data hold them
EDGES = profile.DEFAULT_LAG_EDGES
ANY = len(EDGES) + 1         # 8
ANY_HI = 2 ** 31 - 1


def _digraph():
    # query days: row 0 at 200, row 1 at 130, row 2 (no edge) at 0.  Lags (query day - edge day) and their bins in the comments.
    # row 0: 0 -r0-> 1 (day 198: lag 2, bin 1)  0 -r1-> 2 (day 199: lag 1, bin 0)  0 -r0-> 2 (day 29: lag 171, bin 7)
    #        1 -r4-> 9 (day 139: lag 61, bin 6)  2 -r4-> 9 (day 80: lag 120, bin 6)
    # row 1: 5 -id-> 5 (a self-loop at the window's first day 10: lag 120, written as ANY)  5 -r2-> 7 (day 126: lag 4, bin 2)
    edges = torch.tensor([[0, 1, 0, 0, 1], [0, 1, 0, 1, 2], [0, 1, 0, 0, 2], [0, 2, 1, 4, 9], [0, 2, 2, 4, 9],
                          [1, 1, 5, 6, 5], [1, 2, 5, 2, 7]], dtype=torch.int32)
    alpha = torch.tensor([0.5, 0.25, 0.75, 1.0, 0.5, 0.125, 0.5], dtype=torch.float32)
    return RDigraph(edges=edges, alpha=alpha, offsets=torch.tensor([0, 5, 7, 7]), reached=torch.tensor([True, True, False]),
                    score=torch.zeros(3), n_hops=2, time=torch.tensor([198, 199, 29, 139, 80, 10, 126], dtype=torch.int32),
                    q_time=torch.tensor([200, 130, 0], dtype=torch.int32),
                    data_row=torch.tensor([40, 41, 3, 20, 9, -1, 17], dtype=torch.int32))


def _paths():
    # row 0: (e0, e3) = r0[2-3d] r4[61-120d]; (e2, e4) = r0[121+] r4[61-120d]; (e1, e4) = r1[0-1d] r4[61-120d];  row 1: (e5, e6)
    edge = torch.tensor([[[0, 3], [2, 4], [1, 4]], [[5, 6], [-1, -1], [-1, -1]], [[-1, -1]] * 3])
    product = torch.tensor([[0.5, 0.375, 0.125], [0.0625, 0.0, 0.0], [0.0, 0.0, 0.0]], dtype=torch.float64)
    return PathSet(edge=edge, product=product, count=torch.tensor([3, 1, 0], dtype=torch.int32), digraph=_digraph())


def _same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "lag_bin", "support", "fixed")) \
        and a.n_rel == b.n_rel and a.lag_edges == b.lag_edges


def test_lag_rules_from_paths():
    rd = _digraph()
    assert rd.lag().tolist() == [2, 1, 171, 61, 120, 120, 4]
    assert profile.lag_bins(rd.lag().numpy(), EDGES).tolist() == [1, 0, 7, 6, 6, 6, 2]
    t = lag_rules_from_paths(_paths(), [1, 2, 0], N_REL, EDGES)
    assert isinstance(t, LagRuleTable) and t.lag_edges == EDGES and t.n_rel == N_REL and t.any_bin == ANY
    # sorted by (head, r_1, b_1, r_2, b_2); the identity step of row 1 is ANY although its self-loop has lag 120 (bin 6)
    assert t.head.tolist() == [1, 1, 1, 2]
    assert t.body.tolist() == [[0, 4], [0, 4], [1, 4], [6, 2]]
    assert t.lag_bin.tolist() == [[1, 6], [7, 6], [0, 6], [ANY, 2]]
    assert t.support.tolist() == [1, 1, 1, 1]
    assert t.fixed.tolist() == [int(0.5 * 2 ** 32), int(0.375 * 2 ** 32), int(0.125 * 2 ** 32), int(0.0625 * 2 ** 32)]
    assert t.product_sum().tolist() == [0.5, 0.375, 0.125, 0.0625] and t.mean().tolist() == [0.5, 0.375, 0.125, 0.0625]
    assert t.key().tolist()[0] == [1, 0, 1, 4, 6] and t.key().tolist() == sorted(t.key().tolist())
    # equal keys merge: the same row once more, under the same query relation
    ps = _paths()
    twice = PathSet(torch.cat([ps.edge[:1], ps.edge[:1]]), torch.cat([ps.product[:1], ps.product[:1]]),
                    torch.cat([ps.count[:1], ps.count[:1]]), ps.digraph)
    m = lag_rules_from_paths(twice, [1, 1], N_REL, EDGES)
    assert m.head.tolist() == [1, 1, 1] and m.support.tolist() == [2, 2, 2] and m.fixed.tolist() == [2 * x for x in t.fixed.tolist()[:3]]
    # other edges, other bins: (3, 100) has the bins 0-2d, 3-99d, 100+d; lags 120 and 171 share the last one
    o = lag_rules_from_paths(_paths(), [1, 2, 0], N_REL, (3, 100))
    assert o.lag_edges == (3, 100) and o.any_bin == 3
    assert o.key().tolist() == [[1, 0, 0, 4, 1], [1, 0, 2, 4, 2], [1, 1, 0, 4, 2], [2, 6, 3, 2, 1]]
    # each path is rounded once, to the nearest unit of 2^-32 (halves up), as rules_from_paths rounds
    ps.product[0] = torch.tensor([1.5 * 2.0 ** -32, 2.0 ** -33, 0.49 * 2.0 ** -32], dtype=torch.float64)
    assert lag_rules_from_paths(ps, [1, 2, 0], N_REL, EDGES).fixed.tolist() == [2, 1, 0, int(0.0625 * 2 ** 32)]
    with pytest.raises(ValueError):
        lag_rules_from_paths(_paths(), [1, 2], N_REL, EDGES)
    with pytest.raises(ValueError):
        lag_rules_from_paths(_paths(), [1, 2, 7], N_REL, EDGES)
    with pytest.raises(ValueError, match="lag_edges"):
        lag_rules_from_paths(_paths(), [1, 2, 0], N_REL, (4, 2))
    static = _paths()
    static.digraph.time = None
    with pytest.raises(ValueError, match="static r-digraph"):
        lag_rules_from_paths(static, [1, 2, 0], N_REL, EDGES)
    none = lag_rules_from_paths(PathSet(ps.edge[2:], ps.product[2:], ps.count[2:], ps.digraph), [0], N_REL, EDGES)
    assert none.head.numel() == 0 and none.body.shape == (0, 2) and none.lag_bin.shape == (0, 2) and none.format() == []


def test_format_ranges_top_and_cpu():
    t = lag_rules_from_paths(_paths(), [1, 2, 0], N_REL, EDGES)
    assert t.format() == ["r0[2-3d](x,z1) ^ r4[61-120d](z1,y) -> r1(x,y)", "r0[121+d](x,z1) ^ r4[61-120d](z1,y) -> r1(x,y)",
                          "r1[0-1d](x,z1) ^ r4[61-120d](z1,y) -> r1(x,y)", "r2[4-7d](x,y) -> r2(x,y)"]
    names = ["born", "lives", "works", "born_inv", "lives_inv", "works_inv"]
    assert t.format(names)[3] == "works[4-7d](x,y) -> works(x,y)"
    only_pad = LagRuleTable(torch.tensor([1, 0]), torch.tensor([[6, 6], [3, 6]]), torch.tensor([[ANY, ANY], [ANY, ANY]]),
                            torch.tensor([1, 1]), torch.tensor([5, 5]), EDGES, N_REL)
    assert only_pad.format() == ["x=y -> r1(x,y)", "r3(x,y) -> r0(x,y)"]             # no tag for ANY
    one_day = LagRuleTable(torch.tensor([0]), torch.tensor([[2]]), torch.tensor([[1]]), torch.tensor([1]), torch.tensor([1]), (1, 2), N_REL)
    assert one_day.format() == ["r2[1d](x,y) -> r0(x,y)"]
    # the days of every step: the bins of profile.lag_bins, the last bin and ANY open-ended, ANY from day 0
    lo, hi = t.lag_ranges()
    assert lo.dtype == hi.dtype == torch.int64
    assert lo.tolist() == [[2, 61], [121, 61], [0, 61], [0, 4]] and hi.tolist() == [[4, 121], [ANY_HI, 121], [2, 121], [ANY_HI, 8]]
    for b in range(ANY):                                                             # every lag of a bin lies in the bin's range
        tb = LagRuleTable(torch.tensor([0]), torch.tensor([[0]]), torch.tensor([[b]]), torch.tensor([1]), torch.tensor([1]), EDGES, N_REL)
        (l,), (h,) = (x.reshape(-1).tolist() for x in tb.lag_ranges())
        lags = np.arange(0, 400)
        assert np.array_equal(profile.lag_bins(lags, EDGES) == b, (lags >= l) & (lags < h))
    t.support[:] = torch.tensor([2, 5, 5, 1])
    top = t.top(1, 2)
    assert top.body.tolist() == [[0, 4], [1, 4]] and top.lag_bin.tolist() == [[7, 6], [0, 6]] and top.support.tolist() == [5, 5]
    assert top.lag_edges == EDGES and t.top(2, 5).head.tolist() == [2] and t.top(4, 1).head.numel() == 0
    with pytest.raises(ValueError):
        t.top(1, 0)
    assert _same(t.cpu(), t)
    with pytest.raises(ValueError, match="lag_edges"):
        LagRuleTable(t.head, t.body, t.lag_bin, t.support, t.fixed, (5, 5), N_REL)


def test_add_is_the_table_of_the_concatenation():
    rng = np.random.default_rng(0)
    rd = _digraph()
    B, k, E = 40, 3, rd.edges.shape[0]
    rd.q_time = torch.from_numpy(rng.integers(199, 400, B).astype(np.int32))        # lags are read per edge, whatever the row
    rd.edges[:, 0] = torch.from_numpy(rng.integers(0, B, E).astype(np.int32))
    edge = torch.from_numpy(rng.integers(0, E, (B, k, 2)))
    count = torch.from_numpy(rng.integers(0, k + 1, B).astype(np.int32))
    edge[torch.arange(k)[None, :] >= count[:, None]] = -1
    product = torch.from_numpy(rng.uniform(0, 1, (B, k)))
    q = rng.integers(0, N_REL, B)
    whole = lag_rules_from_paths(PathSet(edge, product, count, rd), q, N_REL, EDGES)
    parts = None
    for lo, hi in ((0, 7), (7, 8), (8, 30), (30, 40)):
        p = lag_rules_from_paths(PathSet(edge[lo:hi], product[lo:hi], count[lo:hi], rd), q[lo:hi], N_REL, EDGES)
        parts = p if parts is None else parts + p
    assert _same(whole, parts) and whole.support.sum() == count.sum()
    key = whole.key().tolist()
    assert key == sorted(key) and len({tuple(x) for x in key}) == len(key)
    assert ((whole.lag_bin == ANY) == (whole.body == N_REL)).all()                  # identity -> ANY, and nothing else is
    empty = lag_rules_from_paths(PathSet(edge[:0], product[:0], count[:0], rd), q[:0], N_REL, EDGES)
    assert _same(whole + empty, whole) and _same(empty + whole, whole)
    with pytest.raises(ValueError, match="do not add"):
        whole + LagRuleTable(whole.head, whole.body, whole.lag_bin, whole.support, whole.fixed, EDGES, N_REL + 2)
    with pytest.raises(ValueError, match="do not add"):
        whole + LagRuleTable(whole.head, whole.body, whole.lag_bin, whole.support, whole.fixed, EDGES[:-1] + (200,), N_REL)
    with pytest.raises(ValueError, match="do not add"):
        whole + LagRuleTable(whole.head, whole.body[:, :1], whole.lag_bin[:, :1], whole.support, whole.fixed, EDGES, N_REL)
    with pytest.raises(TypeError):
        whole + RuleTable(whole.head, whole.body, whole.support, whole.fixed, N_REL)
    with pytest.raises(TypeError):
        whole + TemporalRuleTable(whole.head, whole.body, whole.lag_bin, whole.support, whole.fixed, N_REL)


def _quality():
    head = torch.tensor([0, 0, 0, 0, 1, 0])
    body = torch.tensor([[6, 0], [0, 6], [6, 0], [2, 3], [6, 1], [1, 3]])
    bins = torch.tensor([[ANY, 0], [0, ANY], [ANY, 1], [0, 2], [ANY, 1], [ANY, ANY]])
    one = torch.ones(6, dtype=torch.int64)
    table = LagRuleTable(head, body, bins, one, one.clone(), EDGES, N_REL)
    t = lambda *x: torch.tensor(x, dtype=torch.int64)
    return LagRuleQuality(table, body_pairs=t(8, 8, 10, 4, 3, 0), hits=t(8, 8, 5, 2, 3, 0), pca_body_pairs=t(8, 8, 5, 4, 3, 0),
                          head_pairs=t(8, 8, 8, 8, 3, 8), n_anchors=7)


def test_lag_rule_quality():
    q = _quality()
    assert q.confidence().tolist() == [1.0, 1.0, 0.5, 0.5, 1.0, 0.0]
    assert q.pca_confidence().tolist() == [1.0, 1.0, 1.0, 0.5, 1.0, 0.0]
    assert q.head_coverage().tolist() == [1.0, 1.0, 0.625, 0.25, 1.0, 0.0]
    # no window holds a fact of the query day: the head relation as the only step, however recent, is a real rule
    assert q.trivial().tolist() == [False] * 6 and q.trivial().dtype == torch.bool
    assert q.top(0, 5).tolist() == [1, 0, 2, 3]                 # confidence 1, 1, .5, .5; ties: larger hits, then the smaller (r, bin) key
    assert q.top(0, 5, by="hits").tolist() == [1, 0, 2, 3]
    assert q.top(0, 1).tolist() == [1]                          # rows 0 and 1 tie on score and hits: (0, 0, 6, 8) < (6, 8, 0, 0)
    assert q.top(0, 9, min_hits=0).tolist() == [1, 0, 2, 3, 5] and q.top(1, 3).tolist() == [4]
    with pytest.raises(ValueError):
        q.top(0, 3, by="support")
    lines = q.format()
    assert lines[2] == "r0[2-3d](x,y) -> r0(x,y)  5/10 conf=0.5000 pca=1.0000" and len(lines) == 6
    c = q.cpu()
    assert isinstance(c, LagRuleQuality) and c.n_anchors == 7 and torch.equal(c.hits, q.hits) and c.table.lag_edges == EDGES
    assert RuleQuality.confidence is LagRuleQuality.confidence and RuleQuality.top is LagRuleQuality.top


def test_header_and_binding_carry_the_symbol():
    from red_gnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redgnn.h")).read(), flags=re.S)
    assert re.search(r"\brg_xrule_ground\s*\(", text) and "rg_xrule_ground" in _lib.SYMBOLS
    assert "rg_xrule_ground_scratch_bytes" not in text                  # the scratch is rg_rule_ground_scratch_bytes': no new size function
    L = _lib.lib()
    assert hasattr(L, "rg_xrule_ground") and len(L.rg_xrule_ground.argtypes) == 19
    with pytest.raises(_lib.NativeError, match="rg_xrule_ground: NULL graph"):
        _lib.check(L.rg_xrule_ground(None, None, None, None, None, 1, 1, None, 1, None, None, 1, 120, None, None, 1, None, None, None))


def test_engine_validates_on_the_host():
    from red_gnn_amd import engine
    n_data = 6
    g = types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=n_data + 1)            # no handle, no device: validation never asks for them
    head, body = np.array([0, 1]), np.array([[0, 3], [2, 1]])
    lo, hi = np.array([[0, 0], [2, 121]]), np.array([[2, ANY_HI], [4, ANY_HI]])
    row_day = np.array([0, 0, 1, 3, 3, 4])
    win_lo, win_hi = np.zeros(6, np.int64), np.array([0, 1, 2, 0, 4, 5])
    anchors = np.array([[0, 0], [4, 5]])
    cases = [
        ("head must be", dict(body=body[:1])),
        ("head must be", dict(lag_lo=lo[:, :1])),
        ("head must be", dict(lag_hi=hi[:1])),
        ("must be int32 or int64", dict(lag_lo=lo.astype(np.float64))),
        ("must be int32 or int64", dict(row_day=row_day.astype(np.float32))),
        ("must be int32 or int64", dict(anchors=anchors.astype(np.float32))),
        ("body length 33", dict(body=np.zeros((2, 33), np.int64), lag_lo=np.zeros((2, 33), np.int64), lag_hi=np.ones((2, 33), np.int64))),
        ("not the extrapolation layout", dict(graph=types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=0))),
        ("not the extrapolation layout", dict(graph=types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=12))),
        ("not the extrapolation layout", dict(row_day=row_day[:5])),
        (r"win_lo and win_hi must be \[n_day\]", dict(win_lo=win_lo[:5])),
        (r"win_lo and win_hi must be \[n_day\]", dict(win_lo=win_lo[:0], win_hi=win_hi[:0])),
        ("window bound out of range", dict(win_hi=win_hi + 2)),
        ("loop_window must be", dict(loop_window=-1)),
        ("loop_window must be", dict(loop_window=1.5)),
        (r"relation id out of range 0\.\.3", dict(body=np.array([[0, 4], [2, 1]]))),
        (r"relation id out of range 0\.\.3", dict(head=np.array([0, -1]))),
        ("lag range out of order", dict(lag_lo=np.array([[-1, 0], [2, 121]]))),
        ("lag range out of order", dict(lag_lo=np.array([[2, 0], [2, 121]]))),          # lag_lo == lag_hi
        ("lag range out of order", dict(lag_hi=np.array([[2, 2 ** 31], [4, 200]]))),
        (r"row_day out of range 0\.\.5", dict(row_day=np.array([0, 0, 1, 3, 3, 6]))),
        (r"anchors must be \[S, 2\]", dict(anchors=np.array([0, 1, 2]))),
        ("anchor out of range", dict(anchors=np.array([[5, 0]]))),
        ("anchor out of range", dict(anchors=np.array([[0, 6]]))),
        ("anchor out of range", dict(anchors=np.array([[-1, 0]]))),
        ("duplicate anchors", dict(anchors=np.array([[1, 2], [0, 0], [1, 2]]))),
        ("no longer holds its rows", dict(anchors=None)),
        ("scratch_bytes must be", dict(scratch_bytes=-1)),
        ("scratch_bytes must be", dict(scratch_bytes=1.5)),
        ("scratch_bytes must be", dict(scratch_bytes=True)),
    ]
    for match, change in cases:
        kw = dict(graph=g, head=head, body=body, lag_lo=lo, lag_hi=hi, row_day=row_day, win_lo=win_lo, win_hi=win_hi, anchors=anchors)
        kw.update(change)
        with pytest.raises(ValueError, match="xrule_ground: .*" + match):
            engine.xrule_ground(**kw)
    # what validation hands on: int32 arrays and the anchors sorted by (day, entity)
    out = engine.check_xrules(g, head, torch.as_tensor(body), lo, hi, row_day, win_lo, win_hi, np.array([[4, 2], [1, 0], [0, 2], [3, 0]]))
    assert all(x.dtype == np.int32 for x in out[:7]) and out[7].tolist() == [[1, 0], [3, 0], [0, 2], [4, 2]]
    assert out[3].tolist() == hi.tolist()
    # the default anchors: the distinct (subject, day) of the data rows the graph was built from, the self-loops left out
    rows = np.array([[0, 3, 0, 6], [1, 3, 1, 6], [2, 0, 1, 0], [2, 1, 3, 1], [0, 0, 1, 2], [2, 2, 4, 3], [0, 1, 1, 4], [4, 0, 0, 5]], np.int32)
    g2 = types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=n_data + 1, _rows=(rows, None))
    assert engine.xrule_default_anchors(g2, row_day).tolist() == [[2, 0], [0, 1], [0, 3], [2, 3], [4, 4]]
    assert engine.check_xrules(g2, head, body, lo, hi, row_day, win_lo, win_hi)[7].tolist() == [[2, 0], [0, 1], [0, 3], [2, 3], [4, 4]]
