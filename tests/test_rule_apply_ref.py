"""tests/rule_apply_ref.py against values counted by hand and against itself (dense = sparse, any cut of the rules into ranges), and
the host side of engine.rule_apply: its validation errors and the chunking.  No GPU."""
import numpy as np
import pytest

from tests import rule_apply_ref as A
from tests import rule_ground_ref as G


def _random_case(seed, n_ent=40, n_rel=3, n_facts=90, n_rules=30, L=2, B=50):
    rng = np.random.default_rng(seed)
    n_rela = 2 * n_rel + 1
    trip = np.stack([rng.integers(0, n_ent, n_facts), rng.integers(0, n_rel, n_facts), rng.integers(0, n_ent, n_facts)], 1)
    rows = G.rows_from_triples(n_ent, n_rel, trip)
    head, body = np.sort(rng.integers(0, n_rela, n_rules)), rng.integers(0, n_rela, (n_rules, L))
    weight = rng.integers(1, 65, n_rules).astype(np.float32) / np.float32(64)
    subs, rels = rng.integers(0, n_ent, B), rng.integers(0, n_rela, B)
    return n_ent, n_rela, rows, head, body, weight, subs, rels


def test_hand_graph():
    """The typed-in cells of A.HAND_CELLS, worked out from the A_r sets listed in tests/rule_ground_ref.py."""
    got = A.apply_dense(G.HAND_N_ENT, 5, G.hand_rows(), A.HAND_HEAD, A.HAND_BODY, A.HAND_WEIGHT, A.HAND_SUBS, A.HAND_RELS)
    exp = A.hand_expected()
    assert A.same(got, exp)
    assert got[3][0].tolist() == [0, 0, 1, 0, 0]                                 # (0, r1) under r0 ^ r1 -> r1 reaches exactly entity 2
    assert not got[3][6].any() and (got[1][6] == 1).all()                        # the query whose relation has no rule
    assert np.array_equal(A.scores(got[0], got[1], "noisy_or")[2], np.array([1.0, 0.9375, 0, 0, 0], np.float32))
    assert np.array_equal(A.scores(got[0], got[1], "max")[2], np.array([1.0, 0.75, 0, 0, 0], np.float32))
    assert A.order(A.scores(got[0], got[1], "max")[1], drop=[3]).tolist() == [1, 2, 0, 4]


def test_hand_graph_sparse():
    cells = A.apply_cells(G.HAND_N_ENT, 5, G.hand_rows(), A.HAND_HEAD, A.HAND_BODY, A.HAND_WEIGHT, A.HAND_SUBS, A.HAND_RELS)
    assert len(cells) == len(A.HAND_CELLS)
    assert A.same(A.cells_to_dense(cells, len(A.HAND_SUBS), G.HAND_N_ENT), A.hand_expected())


@pytest.mark.parametrize("seed,L", [(1, 1), (2, 2), (3, 3)])
def test_dense_equals_sparse(seed, L):
    c = _random_case(seed, L=L)
    dense = A.apply_dense(*c)
    assert A.same(dense, A.cells_to_dense(A.apply_cells(*c), len(c[6]), c[0]))
    assert (dense[3] >= 2).any() and (dense[3] == 0).any()


@pytest.mark.parametrize("cuts", [(0, 30), (0, 1, 30), (0, 7, 8, 19, 30), tuple(range(31))])
def test_cutting_the_rules_changes_nothing(cuts):
    n_ent, n_rela, rows, head, body, weight, subs, rels = _random_case(4)
    whole = A.apply_dense(n_ent, n_rela, rows, head, body, weight, subs, rels)
    assert len(np.unique(head)) < 30                     # so cutting before every rule cuts inside a head's rules
    state, cells = None, None
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        state = A.apply_dense(n_ent, n_rela, rows, head[lo:hi], body[lo:hi], weight[lo:hi], subs, rels, state, lo)
        cells = A.apply_cells(n_ent, n_rela, rows, head[lo:hi], body[lo:hi], weight[lo:hi], subs, rels, cells, lo)
    assert A.same(state, whole) and A.same(A.cells_to_dense(cells, len(subs), n_ent), whole)


def test_noisy_or_is_at_least_max():
    best, surv, rule, fired = A.apply_dense(*_random_case(5, n_rules=60))
    nor, mx = A.scores(best, surv, "noisy_or"), A.scores(best, surv, "max")
    hit = fired > 0
    assert hit.any() and (~hit).any() and (fired >= 3).any()
    assert (nor[hit] >= mx[hit]).all() and (mx[hit] > 0).all() and (rule[hit] >= 0).all()
    assert (nor[~hit] == 0).all() and (mx[~hit] == 0).all() and (rule[~hit] == -1).all()


# ---- engine: host validation and chunking (no device is touched before they pass) ---------------------------------------------
class _Graph:
    n_ent, n_rel, n_time, device = 5, 2, 0, "cuda"


def test_host_validation_errors():
    from red_gnn_amd import engine
    ok = dict(head=A.HAND_HEAD, body=A.HAND_BODY, weight=A.HAND_WEIGHT, subs=A.HAND_SUBS, rels=A.HAND_RELS)

    def check(match, **kw):
        a = dict(ok, **kw)
        with pytest.raises(ValueError, match=match):
            engine.rule_apply(_Graph(), a["head"], a["body"], a["weight"], a["subs"], a["rels"])

    check("rule_apply: head must be non-decreasing", head=A.HAND_HEAD[::-1].copy())
    check(r"rule_apply: relation id out of range 0\.\.4", body=A.HAND_BODY + 1)
    check("rule_apply: head must be \\[R\\] and body \\[R, L\\]", body=A.HAND_BODY[:3])
    check("rule_apply: the body length 33 is not in 1..32", body=np.zeros((6, 33), np.int64))
    for bad in (0.0, 1.5, np.nan, np.inf, -0.25):
        w = A.HAND_WEIGHT.copy()
        w[2] = bad
        check("rule_apply: weights must be finite and in \\(0, 1\\]", weight=w)
    check("rule_apply: weights must be finite and in \\(0, 1\\]", weight=np.full(6, 1e-50))           # 0 as float32
    check("rule_apply: weight must be a float array \\[R\\]", weight=A.HAND_WEIGHT[:5])
    check("rule_apply: weight must be a float array \\[R\\]", weight=np.ones(6, np.int64))
    check("rule_apply: need one relation per subject", rels=A.HAND_RELS[:3])
    check(r"rule_apply: subject id out of range 0\.\.4", subs=A.HAND_SUBS + 2)
    check(r"rule_apply: query relation id out of range 0\.\.4", rels=A.HAND_RELS - 1)
    check("rule_apply: subs must be int32 or int64", subs=A.HAND_SUBS.astype(np.float64))
    with pytest.raises(ValueError, match="rule_apply: scratch_bytes must be a non-negative integer"):
        engine.rule_apply(_Graph(), scratch_bytes=-1, **ok)

    class Temporal(_Graph):
        n_time = 3
    with pytest.raises(ValueError, match="rule_apply: temporal graph"):
        engine.rule_apply(Temporal(), **ok)
    h, b, w, s, r = engine.check_rule_apply(5, 2, **ok)
    assert [a.dtype for a in (h, b, w, s, r)] == [np.int32, np.int32, np.float32, np.int32, np.int32]


def test_chunking():
    from red_gnn_amd import engine
    rng = np.random.default_rng(6)
    bytes_of = engine.rule_apply_scratch_bytes
    assert bytes_of(0) == 0 and bytes_of(1) == 512 and bytes_of(64) == 512 and bytes_of(65) == 1024 and bytes_of((1 << 40) + 1) == 0
    for trial in range(40):
        R = int(rng.integers(1, 60))
        words = (rng.integers(0, 4, R) * rng.integers(1, 500, R)).astype(np.int64)
        budget = int(rng.integers(0, 4 * 4 * int(words.sum()) + 600))
        chunks = engine.rule_apply_chunking(words, budget)
        assert [lo for lo, _ in chunks] == [0] + [hi for _, hi in chunks[:-1]] and chunks[-1][1] == R       # covers 0..R in order
        for k, (lo, hi) in enumerate(chunks):
            assert hi > lo
            total = int(words[lo:hi].sum())
            assert hi - lo == 1 or bytes_of(max(total, 1)) <= budget                                       # fits, or a single rule
            if hi < R:                                                                                     # greedy: the next did not fit
                assert bytes_of(max(total + int(words[hi]), 1)) > budget
    assert engine.rule_apply_chunking(np.array([10, 10, 10]), 1 << 30) == [(0, 3)]
    assert engine.rule_apply_chunking(np.array([100, 100, 100]), 0) == [(0, 1), (1, 2), (2, 3)]
    assert engine.rule_apply_chunking(np.zeros(0, np.int64), 1 << 30) == []
    many = engine.rule_apply_chunking(np.ones(70000, np.int64), 1 << 30)
    assert many == [(0, engine.RULE_MAX_RULES), (engine.RULE_MAX_RULES, 70000)]
