"""CPU-only checks of the code the rule families share on the host, reached through every caller: the generic cpu() of the tables and
the qualities, __add__ / top / format of the two step tables, and the whole error texts of the engine's shared checks under every
family's name.  Hand-sized tables with L = 2; the expected tensors and strings are literal."""
import types

import numpy as np
import pytest
import torch

from red_gnn_amd import engine
from red_gnn_amd.explain import LagRuleQuality, LagRuleTable, RuleQuality, RuleTable, TemporalRuleQuality, TemporalRuleTable

T = lambda x: torch.tensor(x, dtype=torch.int64)
EDGES = (1, 2, 4)            # lag bins [0d] [1d] [2-3d] [4+d], ANY = 4


def _temporal():
    return (TemporalRuleTable(T([0, 0, 1]), T([[1, 2], [3, 2], [0, 3]]), T([[0, 1], [2, 3], [1, 3]]), T([2, 5, 1]), T([10, 20, 30]), 3),
            TemporalRuleTable(T([0, 1]), T([[3, 2], [1, 1]]), T([[2, 3], [0, 0]]), T([1, 4]), T([5, 6]), 3))


def _lag():
    return (LagRuleTable(T([0, 0, 1]), T([[1, 2], [3, 2], [0, 3]]), T([[0, 1], [2, 4], [3, 4]]), T([2, 5, 1]), T([10, 20, 30]), EDGES, 3),
            LagRuleTable(T([0, 1]), T([[3, 2], [1, 1]]), T([[2, 4], [0, 0]]), T([1, 4]), T([5, 6]), EDGES, 3))


def _fields(x):
    """Every field of a table or quality as plain Python: tensors as (dtype, list), tables recursively."""
    out = []
    for name in x.__dataclass_fields__:
        v = getattr(x, name)
        out.append((name, (v.dtype, v.is_contiguous(), v.tolist()) if torch.is_tensor(v) else (_fields(v) if hasattr(v, "head") else v)))
    return out


@pytest.mark.parametrize("tables,step,steps,lines", [
    (_temporal, "direction", [[0, 1], [2, 3], [1, 3], [0, 0]],
     ["r1[past](x,z1) ^ r2[now](z1,y) -> r0(x,y)", "r2(x,y) -> r0(x,y)", "r0[now](x,y) -> r1(x,y)",
      "r1[past](x,z1) ^ r1[past](z1,y) -> r1(x,y)"]),
    (_lag, "lag_bin", [[0, 1], [2, 4], [3, 4], [0, 0]],
     ["r1[0d](x,z1) ^ r2[1d](z1,y) -> r0(x,y)", "r2(x,y) -> r0(x,y)", "r0[4+d](x,y) -> r1(x,y)", "r1[0d](x,z1) ^ r1[0d](z1,y) -> r1(x,y)"]),
])
def test_step_tables_add_top_format_and_cpu(tables, step, steps, lines):
    t, u = tables()
    s = t + u
    assert type(s) is type(t) and s.n_rel == 3 and list(s.__dataclass_fields__) == list(t.__dataclass_fields__)
    assert s.head.tolist() == [0, 0, 1, 1] and s.body.tolist() == [[1, 2], [3, 2], [0, 3], [1, 1]]
    assert getattr(s, step).tolist() == steps and s.support.tolist() == [2, 6, 1, 4] and s.fixed.tolist() == [10, 25, 30, 6]
    assert all(x.dtype == torch.int64 and x.is_contiguous() for x in (s.head, s.body, getattr(s, step), s.support, s.fixed))
    assert s.key().tolist() == [[0, 1, steps[0][0], 2, steps[0][1]], [0, 3, steps[1][0], 2, steps[1][1]],
                                [1, 0, steps[2][0], 3, steps[2][1]], [1, 1, 0, 1, 0]]
    assert s.format() == lines and s.format(["a", "b", "c", "d"])[0] == lines[0].replace("r1", "b").replace("r2", "c").replace("r0", "a")
    assert s.product_sum().tolist() == [10 * 2.0 ** -32, 25 * 2.0 ** -32, 30 * 2.0 ** -32, 6 * 2.0 ** -32]
    top = t.top(0, 1)
    assert type(top) is type(t) and _fields(top)[:5] == [("head", (torch.int64, True, [0])), ("body", (torch.int64, True, [[3, 2]])),
                                                         (step, (torch.int64, True, [steps[1]])), ("support", (torch.int64, True, [5])),
                                                         ("fixed", (torch.int64, True, [20]))]
    assert _fields(top)[5:] == _fields(t)[5:] and s.top(1, 5).support.tolist() == [4, 1] and s.top(2, 1).head.numel() == 0
    with pytest.raises(ValueError, match=r"^top: n must be a positive integer \(got 0\)$"):
        t.top(0, 0)
    with pytest.raises(ValueError, match=r"^top: n must be a positive integer \(got True\)$"):
        t.top(0, True)
    c = t.cpu()
    assert type(c) is type(t) and c is not t and _fields(c) == _fields(t) and repr(c) == repr(t)
    assert t.__add__(RuleTable(t.head, t.body, t.support, t.fixed, 3)) is NotImplemented


def test_step_tables_that_do_not_add():
    t, _ = _temporal()
    with pytest.raises(ValueError) as e:
        t + TemporalRuleTable(t.head, t.body, t.direction, t.support, t.fixed, 4)
    assert str(e.value) == "rule tables of different relation count or path length do not add (n_rel 3 / 4, L 2 / 2)"
    with pytest.raises(ValueError) as e:
        t + TemporalRuleTable(t.head, t.body[:, :1], t.direction[:, :1], t.support, t.fixed, 3)
    assert str(e.value) == "rule tables of different relation count or path length do not add (n_rel 3 / 3, L 2 / 1)"
    lt, _ = _lag()
    with pytest.raises(ValueError) as e:
        lt + LagRuleTable(lt.head, lt.body, lt.lag_bin, lt.support, lt.fixed, (1, 2), 3)
    assert str(e.value) == ("rule tables of different relation count, path length or lag edges do not add (n_rel 3 / 3, L 2 / 2, "
                            "lag_edges (1, 2, 4) / (1, 2))")
    with pytest.raises(TypeError):
        t + lt


def test_every_quality_has_the_generic_cpu_and_its_own_fields():
    r = RuleTable(T([0, 1]), T([[1, 2], [0, 6]]), T([2, 1]), T([7, 9]), 3)
    t, lt = _temporal()[0], _lag()[0]
    counts = (T([4, 2, 1]), T([2, 1, 0]), T([3, 2, 1]), T([5, 6, 7]))
    cases = [(RuleQuality(r, *(c[:2] for c in counts), 7), "n_sources", 7, ["r1(x,z1) ^ r2(z1,y) -> r0(x,y)  2/4 conf=0.5000 pca=0.6667",
                                                                          "r0(x,y) -> r1(x,y)  1/2 conf=0.5000 pca=0.5000"]),
             (TemporalRuleQuality(t, *counts, 9), "n_anchors", 9, ["r1[past](x,z1) ^ r2[now](z1,y) -> r0(x,y)  2/4 conf=0.5000 pca=0.6667",
                                                                 "r2(x,y) -> r0(x,y)  1/2 conf=0.5000 pca=0.5000",
                                                                 "r0[now](x,y) -> r1(x,y)  0/1 conf=0.0000 pca=0.0000"]),
             (LagRuleQuality(lt, *counts, 11), "n_anchors", 11, ["r1[0d](x,z1) ^ r2[1d](z1,y) -> r0(x,y)  2/4 conf=0.5000 pca=0.6667",
                                                               "r2(x,y) -> r0(x,y)  1/2 conf=0.5000 pca=0.5000",
                                                               "r0[4+d](x,y) -> r1(x,y)  0/1 conf=0.0000 pca=0.0000"])]
    for q, last, n, lines in cases:
        assert list(q.__dataclass_fields__) == ["table", "body_pairs", "hits", "pca_body_pairs", "head_pairs", last]
        c = q.cpu()
        assert type(c) is type(q) and type(c.table) is type(q.table) and c is not q and c.table is not q.table
        assert _fields(c) == _fields(q) and getattr(c, last) == n and repr(c) == repr(q)
        assert repr(q).startswith(type(q).__name__ + "(table=" + type(q.table).__name__ + "(head=tensor([0, ")
        assert repr(q).endswith("head_pairs=tensor(%s), %s=%d)" % (q.head_pairs.tolist(), last, n))
        assert q.format() == lines and q.confidence().tolist()[:2] == [0.5, 0.5]
    assert repr(r.cpu()) == repr(r) and _fields(r.cpu()) == _fields(r) and r.cpu() is not r


def _message(f, *args, **kw):
    with pytest.raises(ValueError) as e:
        f(*args, **kw)
    return str(e.value)


def test_shared_engine_checks_keep_every_family_s_text():
    head, body, direc = np.array([0, 1]), np.array([[0, 6], [2, 3]]), np.array([[0, 3], [1, 2]])
    g = types.SimpleNamespace(n_ent=5, n_rela_rows=7, n_time=3)
    tr = lambda a: _message(engine.check_trules, g, head, body, direc, a)
    assert tr(np.array([0, 1, 2])) == "trule_ground: anchors must be [S, 2] = (entity, time id) (got (3,))"
    assert tr(np.array([[5, 0]])) == "trule_ground: anchor out of range (entity 0..4, time id 0..2; got 5..5 and 0..0)"
    assert tr(np.array([[0, 3]])) == "trule_ground: anchor out of range (entity 0..4, time id 0..2; got 0..0 and 3..3)"
    assert tr(np.array([[1, 2], [0, 0], [1, 2]])) == "trule_ground: duplicate anchors (3 pairs, 2 distinct)"
    assert _message(engine.check_trules, g, head, body[:1], direc) == \
        "trule_ground: head must be [R], body and direction [R, L] (got (2,), (1, 2) and (2, 2))"
    assert _message(engine.check_trules, g, head, np.array([[0, 7], [2, 3]]), direc) == "trule_ground: relation id out of range 0..6 (got 0..7)"
    assert engine.check_trules(g, head, body, direc, np.array([[4, 2], [1, 0], [0, 2]]))[3].tolist() == [[1, 0], [0, 2], [4, 2]]

    gx = types.SimpleNamespace(n_ent=5, n_rela_rows=4, n_time=7)
    bx, lo, hi = np.array([[0, 3], [2, 1]]), np.array([[0, 0], [2, 121]]), np.array([[2, 200], [4, 200]])
    day, wl, wh = np.array([0, 0, 1, 3, 3, 4]), np.zeros(6, np.int64), np.array([0, 1, 2, 0, 4, 5])
    xr = lambda a, b=bx, lag_lo=lo: _message(engine.check_xrules, gx, head, b, lag_lo, hi, day, wl, wh, a)
    assert xr(np.array([0, 1, 2])) == "xrule_ground: anchors must be [S, 2] = (entity, day) (got (3,))"
    assert xr(np.array([[5, 0]])) == "xrule_ground: anchor out of range (entity 0..4, day 0..5; got 5..5 and 0..0)"
    assert xr(np.array([[0, 6]])) == "xrule_ground: anchor out of range (entity 0..4, day 0..5; got 0..0 and 6..6)"
    assert xr(np.array([[1, 2], [0, 0], [1, 2]])) == "xrule_ground: duplicate anchors (3 pairs, 2 distinct)"
    assert xr(np.array([[0, 0]]), lag_lo=lo[:, :1]) == \
        "xrule_ground: head must be [R], body, lag_lo and lag_hi [R, L] (got (2,), (2, 2), (2, 1) and (2, 2))"
    assert xr(np.array([[0, 0]]), b=np.array([[0, 4], [2, 1]])) == "xrule_ground: relation id out of range 0..3 (got 0..4)"
    assert engine.check_xrules(gx, head, bx, lo, hi, day, wl, wh, np.array([[4, 2], [1, 0], [0, 2]]))[7].tolist() == [[1, 0], [0, 2], [4, 2]]

    assert _message(engine.check_rules, 5, 3, head, body[:1]) == "rule_ground: head must be [R] and body [R, L] (got (2,) and (1, 2))"
    assert _message(engine.check_rules, 5, 3, head, np.array([[0, 7], [2, 3]])) == \
        "rule_ground: relation id out of range 0..6 (2*n_rel; got 0..7)"
    assert _message(engine.check_rules, 5, 3, head, np.zeros((2, 33), np.int64)) == "rule_ground: the body length 33 is not in 1..32"
    assert _message(engine.check_rule_apply, 5, 3, np.array([1, 0]), body, np.array([.5, .5]), [0], [0]) == \
        "rule_apply: head must be non-decreasing (rule 1 has head 0 after 1)"
    assert _message(engine.check_rule_apply, 5, 3, head, body, np.array([.5, 1.5]), [0], [0]) == \
        "rule_apply: weights must be finite and in (0, 1] as float32 (rule 1 has 1.5)"
    assert _message(engine.check_trule_apply, g, head, body, direc, np.array([.5, 0.0]), [0], [0], [0]) == \
        "trule_apply: weights must be finite and in (0, 1] as float32 (rule 1 has 0.0)"
    assert _message(engine.check_trule_apply, g, head, body, direc, np.array([1, 1]), [0], [0], [0]) == \
        "trule_apply: weight must be a float array [R] (got int64 (2,) for 2 rules)"
    static = types.SimpleNamespace(n_ent=5, n_rel=3, n_time=0)
    assert _message(engine.rule_ground, static, head, body, scratch_bytes=1.5) == \
        "rule_ground: scratch_bytes must be a non-negative integer (got 1.5)"
    assert _message(engine.rule_apply, static, head, body, np.array([.5, .5]), [0], [0], scratch_bytes=True) == \
        "rule_apply: scratch_bytes must be a non-negative integer (got True)"
    assert _message(engine.trule_ground, g, head, body, direc, scratch_bytes=-1) == \
        "trule_ground: scratch_bytes must be a non-negative integer (got -1)"
    assert _message(engine.xrule_ground, gx, head, bx, lo, hi, day, wl, wh, np.array([[0, 0]]), scratch_bytes=-1) == \
        "xrule_ground: scratch_bytes must be a non-negative integer (got -1)"
    assert _message(engine.trule_apply, g, head, body, direc, np.array([.5, .5]), [0], [0], [0], scratch_bytes=-1) == \
        "trule_apply: scratch_bytes must be a non-negative integer (got -1)"
