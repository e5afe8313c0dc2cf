"""engine.trule_apply (rg_trule_apply, csrc/trule_apply.hip) and T_RED_GNN.rule_scores / rule_predict / rule_evaluate on the MI355X
(-m gpu): every output equal bit for bit to tests/trule_apply_ref.py on the quadruples the device graph was built from - the hand graph
with its typed-in cells, a 200-entity graph under 180 random rules of every direction with one relation of more words than a wave,
per-relation query counts around the word boundaries, time ranges that start and end on word boundaries or lie at one end of the time
axis, the row order, the smallest chunking, other path lengths, the counts of rg_trule_ground, slabs past 2^31 words, the model entry
points on the model's hand graph, the errors, and the kernel's own bounds on relation ids, directions and query rows."""
import numpy as np
import pytest
import torch

from tests import layer_ref as LR
from tests import rank_ref
from tests import rule_apply_ref as A
from tests import rule_ground_ref as G
from tests import temporal_ref as TR
from tests import trule_apply_ref as TA
from tests import trule_ground_ref as T

pytestmark = pytest.mark.gpu

BOUNDARY_COUNTS = (1, 31, 32, 33, 64, 65)


def _np(four):
    return tuple(t.cpu().numpy() for t in four)


def _check_types(four, B, n_ent):
    assert all(t.is_cuda and t.shape == (B, n_ent) for t in four)
    assert [t.dtype for t in four] == [torch.float32, torch.float32, torch.int32, torch.int32]


def _weights(rng, n):
    return rng.integers(1, 257, n).astype(np.float32) / np.float32(256)


def _directions(rng, shape):
    """About half "any", the rest past / now / future."""
    return np.where(rng.random(shape) < 0.5, T.ANY, rng.integers(0, 3, shape))


def test_hand_graph():
    from red_gnn_amd import engine
    quads = T.hand_quads()
    g = engine.TemporalGraph(T.HAND_N_ENT, T.HAND_N_RELA, T.HAND_N_TIME, quads)
    rules = (TA.HAND_HEAD, TA.HAND_BODY, TA.HAND_DIR, TA.HAND_WEIGHT)
    queries = (TA.HAND_SUBS, TA.HAND_RELS, TA.HAND_TIMES)
    B = len(TA.HAND_SUBS)
    got = engine.trule_apply(g, *rules, *queries)
    _check_types(got, B, T.HAND_N_ENT)
    assert A.same(_np(got), TA.hand_expected())
    assert A.same(_np(got), TA.apply_dense(T.HAND_N_ENT, T.HAND_N_RELA, T.HAND_N_TIME, quads, *rules, *queries))
    as_t = lambda a: torch.as_tensor(a).cuda()
    again = engine.trule_apply(g, *(as_t(a) for a in rules), *(as_t(a) for a in queries))
    assert A.same(_np(again), TA.hand_expected())
    none = engine.trule_apply(g, *(a[:0] for a in rules), *queries)                                            # R = 0
    _check_types(none, B, T.HAND_N_ENT)
    assert A.same(_np(none), A.initial(B, T.HAND_N_ENT))
    empty = engine.trule_apply(g, *rules, *(a[:0] for a in queries))                                          # B = 0
    _check_types(empty, 0, T.HAND_N_ENT)
    only = engine.trule_apply(g, *rules, *(a[8:] for a in queries))                                           # no rule has a query
    assert A.same(_np(only), A.initial(1, T.HAND_N_ENT))


@pytest.fixture(scope="module")
def case():
    """layer_ref._temporal_case(seed=2, B=9, m=600): 200 entities, 11 relation ids, 12 time ids; its device graph; 2 730 queries - 70
    of every non-identity relation over all times, and 2 030 more of relation ``big``, which so has 2 100 queries = 66 words; 60 rules
    per length 1, 2, 3 with heads among three relations (``big`` one of them), bodies over all ids and about half the directions
    "any"; the reference outputs and, per cell, the first rule that fires, computed once."""
    from red_gnn_amd import engine
    c = LR._temporal_case("trule", seed=2, B=9, m=600)
    n_ent, n_rela, n_time, quads = c.n_ent, c.n_rela_rows, c.n_time, c.quads
    assert (n_ent, n_rela, n_time) == (200, 11, 12)
    graph = engine.TemporalGraph(n_ent, n_rela, n_time, quads)
    rng = np.random.default_rng(23)
    big, heads = 3, np.array([1, 3, 7])
    rels = np.concatenate([np.repeat(np.arange(n_rela - 1), 70), np.full(2030, big)])
    B = len(rels)
    subs, times = rng.integers(0, n_ent, B), rng.integers(0, n_time, B)
    mix = rng.permutation(B)
    subs, rels, times = subs[mix], rels[mix], times[mix]
    assert ((rels == big).sum() + 31) // 32 == 66
    assert len(np.unique(rels * n_time + times)) == (n_rela - 1) * n_time                    # every (relation, time id) has a query
    args = (n_ent, n_rela, n_time, quads)
    rules, ref, first = {}, {}, {}
    for L in (1, 2, 3):
        head = np.sort(rng.choice(heads, 60))
        body, direc, weight = rng.integers(0, n_rela, (60, L)), _directions(rng, (60, L)), _weights(rng, 60)
        rules[L] = (head, body, direc, weight)
        ref[L] = A.cells_to_dense(TA.apply_cells(*args, *rules[L], subs, rels, times), B, n_ent)
        fire = TA.firing_packed(*args, subs, rels, times)
        f = np.full((B, n_ent), -1)
        for i in range(59, -1, -1):
            bi, yi = fire(int(head[i]), body[i].tolist(), direc[i].tolist())
            f[bi, yi] = i
        first[L] = f
    return dict(graph=graph, n_ent=n_ent, n_rela=n_rela, n_time=n_time, quads=quads, args=args, subs=subs, rels=rels, times=times,
                big=big, heads=heads, rules=rules, ref=ref, first=first)


def _ref(c, rules, subs, rels, times):
    return A.cells_to_dense(TA.apply_cells(*c["args"], *rules, subs, rels, times), len(subs), c["n_ent"])


def test_random_rules_equal_the_reference(case):
    from red_gnn_amd import engine
    c = case
    for L, r in c["rules"].items():
        got = engine.trule_apply(c["graph"], *r, c["subs"], c["rels"], c["times"])
        _check_types(got, len(c["subs"]), c["n_ent"])
        assert A.same(_np(got), c["ref"][L]), L
        assert np.array_equal((1.0 - got[1]).cpu().numpy().view(np.int32), A.scores(*c["ref"][L][:2], "noisy_or").view(np.int32))


def test_the_comparison_is_not_one_of_defaults(case):
    c = case
    for L, r in c["rules"].items():
        best, surv, rule, fired = c["ref"][L]
        assert (fired > 0).sum() >= 1000, L
        assert (fired >= 2).sum() >= 100 and (fired >= 3).any(), L
        assert ((rule != c["first"][L]) & (fired >= 2)).any() and ((rule == c["first"][L]) & (fired >= 2)).any(), L
        assert np.array_equal(c["first"][L] >= 0, fired > 0)
        assert set(r[2].reshape(-1).tolist()) == {0, 1, 2, 3} and (r[1] == c["n_rela"] - 1).any() and (r[1] >= 5).any()
        assert (fired[c["rels"] == c["big"]] > 0).any() and (fired[c["rels"] == 1] > 0).any()
        assert not fired[~np.isin(c["rels"], c["heads"])].any()
    # the dense definition itself on a part of the queries (it takes minutes on all of them)
    part = np.arange(0, len(c["subs"]), 23)
    q = (c["subs"][part], c["rels"][part], c["times"][part])
    r = c["rules"][2]
    dense = TA.apply_dense(*c["args"], *r, *q)
    assert A.same(dense, tuple(a[part] for a in c["ref"][2])) and (dense[3] > 0).any()


def test_word_boundaries(case):
    from red_gnn_amd import engine
    c = case
    rng = np.random.default_rng(31)
    ids = rng.permutation(c["n_rela"] - 1)[:len(BOUNDARY_COUNTS)]
    rels = np.concatenate([np.full(n, r) for r, n in zip(ids, BOUNDARY_COUNTS)])
    B = len(rels)
    subs, times = rng.integers(0, c["n_ent"], B), rng.integers(0, c["n_time"], B)
    mix = rng.permutation(B)
    subs, rels, times = subs[mix], rels[mix], times[mix]
    assert sorted(np.bincount(rels, minlength=c["n_rela"])[ids].tolist()) == sorted(BOUNDARY_COUNTS)
    for L in (1, 2):
        rules = (np.sort(rng.choice(ids, 48)), rng.integers(0, c["n_rela"], (48, L)), _directions(rng, (48, L)), _weights(rng, 48))
        assert set(rules[0].tolist()) == set(ids.tolist())
        got = _np(engine.trule_apply(c["graph"], *rules, subs, rels, times))
        ref = _ref(c, rules, subs, rels, times)
        assert A.same(got, ref)
        for r, n in zip(ids, BOUNDARY_COUNTS):
            assert n < 31 or (ref[3][rels == r] > 0).any(), (L, r)            # (a single query may well reach nothing)
        if L == 2:
            assert A.same(got, TA.apply_dense(*c["args"], *rules, subs, rels, times))


def test_time_ranges_on_word_boundaries_and_at_the_ends(case):
    from red_gnn_amd import engine
    c = case
    rng = np.random.default_rng(7)
    n_ent, last, h = c["n_ent"], c["n_time"] - 1, 2
    ents = lambda k: rng.integers(0, n_ent, k)
    at = lambda t, k: (ents(k), np.full(k, h), np.full(k, t))
    cat = lambda *qs: tuple(np.concatenate(x) for x in zip(*qs))
    sets = dict(three_full_words=cat(at(0, 32), at(5, 32), at(last, 32)),         # every range starts and ends on a word boundary
                all_at_time_0=at(0, 70), all_at_last_time=at(last, 70),
                spread=(ents(150), np.full(150, h), rng.integers(0, c["n_time"], 150)))
    for name, q in sets.items():
        for L in (1, 2, 3):
            rules = (np.full(30, h), rng.integers(0, c["n_rela"], (30, L)), _directions(rng, (30, L)), _weights(rng, 30))
            ref = _ref(c, rules, *q)
            assert A.same(_np(engine.trule_apply(c["graph"], *rules, *q)), ref), (name, L)
            assert (ref[3] > 0).any(), (name, L)
    # L = 1, stated outright: one rule per direction over one relation, each applied alone
    rel = 0
    one = lambda d, q: engine.trule_apply(c["graph"], np.array([h]), np.array([[rel]]), np.array([[d]]), np.ones(1, np.float32), *q)[3] \
        .cpu().numpy() > 0
    for name, q in sets.items():
        past, now, future, anyt = (one(d, q) for d in (T.PAST, T.NOW, T.FUTURE, T.ANY))
        assert np.array_equal(now | past | future, anyt) and anyt.any(), name           # cell by cell
        if name == "all_at_time_0":
            assert not past.any() and future.any()                                       # no edge lies before time 0
        if name == "all_at_last_time":
            assert not future.any() and past.any()                                       # none after the last time id
        if name == "spread":
            assert past.any() and now.any() and future.any()


def test_row_order(case):
    from red_gnn_amd import engine
    c = case
    rng = np.random.default_rng(41)
    pick = rng.permutation(len(c["subs"]))[:300]
    subs, rels, times = c["subs"][pick].copy(), c["rels"][pick].copy(), c["times"][pick].copy()
    r = c["rules"][2]
    src = int(np.argmax(_ref(c, r, subs, rels, times)[3].sum(1) > 0))                            # a query some rule answers
    dup = (src, (src + 1) % len(subs))
    subs[dup[1]], rels[dup[1]], times[dup[1]] = subs[dup[0]], rels[dup[0]], times[dup[0]]        # stated twice
    got = engine.trule_apply(c["graph"], *r, subs, rels, times)
    assert A.same(_np(got), _ref(c, r, subs, rels, times)) and bool((got[3] > 0).any())
    assert all(torch.equal(t[dup[0]], t[dup[1]]) for t in got) and bool((got[3][dup[0]] > 0).any())
    perm = rng.permutation(len(subs))
    moved = engine.trule_apply(c["graph"], *r, subs[perm], rels[perm], times[perm])
    at = torch.as_tensor(perm).cuda()
    assert all(torch.equal(a[at], b) for a, b in zip(got, moved))


def test_chunking_changes_no_bit(case):
    from red_gnn_amd import engine
    c = case
    r = c["rules"][3]
    R = len(r[0])
    counts = np.bincount(c["rels"], minlength=c["n_rela"])
    words = c["n_ent"] * ((counts[r[0]] + 31) // 32)
    assert engine.rule_apply_chunking(words, engine.RULE_SCRATCH_BYTES) == [(0, R)]
    assert engine.rule_apply_chunking(words, 0) == [(i, i + 1) for i in range(R)] and len(np.unique(r[0])) < R
    mid_budget = engine.rule_apply_scratch_bytes(int(words[:7].sum()))
    mid_chunks = engine.rule_apply_chunking(words, mid_budget)
    assert 1 < len(mid_chunks) < R and mid_chunks[0] == (0, 7)
    args = (c["graph"], *r, c["subs"], c["rels"], c["times"])
    whole = engine.trule_apply(*args)
    one = engine.trule_apply(*args, scratch_bytes=0)                              # one rule per call: every head's rules are cut apart
    events = engine.TRULE_APPLY_EVENTS = []
    try:
        mid = engine.trule_apply(*args, scratch_bytes=mid_budget)
    finally:
        engine.TRULE_APPLY_EVENTS = None
    assert all(torch.equal(a, b) and torch.equal(a, m) for a, b, m in zip(whole, one, mid))
    assert A.same(_np(whole), c["ref"][3])
    assert [(e[3], e[4]) for e in events] == [(r1 - r0, int(words[r0:r1].sum())) for r0, r1 in mid_chunks]


@pytest.mark.parametrize("L", [1, 4])
def test_path_lengths(case, L):
    from red_gnn_amd import engine
    c = case
    rng = np.random.default_rng(200 + L)
    pick = np.arange(0, len(c["subs"]), 5)
    q = (c["subs"][pick], c["rels"][pick], c["times"][pick])
    rules = (np.sort(rng.integers(0, c["n_rela"], 30)), rng.integers(0, c["n_rela"], (30, L)), _directions(rng, (30, L)), _weights(rng, 30))
    ref = _ref(c, rules, *q)
    assert A.same(_np(engine.trule_apply(c["graph"], *rules, *q)), ref)
    assert (ref[3] > 0).any() and (ref[3] == 0).any()


def test_agrees_with_trule_ground(case):
    """Distinct (s, t) queries of one relation h are anchors: a single rule of head h fires for as many cells as rg_trule_ground
    counts body pairs, and the fired cells that are facts (s, h, y, t) of the graph number its hits."""
    from red_gnn_amd import engine
    c = case
    rng = np.random.default_rng(51)
    h = 1
    anchors = T.default_anchors(c["quads"], c["n_ent"], c["n_rela"])
    anchors = anchors[rng.permutation(len(anchors))[:400]]
    subs, times = anchors[:, 0], anchors[:, 1]
    facts = set(map(tuple, c["quads"][c["quads"][:, 1] == h][:, [0, 2, 3]].tolist()))
    some_hits = 0
    for L in (1, 2, 3):
        for n in range(4):
            body, direc = rng.integers(0, c["n_rela"], (1, L)), _directions(rng, (1, L))
            if L == 1 and n == 0:
                body, direc = np.array([[h]]), np.array([[T.NOW]])                    # the head itself: every body pair is a hit
            fired = engine.trule_apply(c["graph"], np.array([h]), body, direc, np.ones(1, np.float32), subs, np.full(len(subs), h), times)[3]
            counts = engine.trule_ground(c["graph"], np.array([h]), body, direc, anchors).cpu().numpy()[0]
            b, y = np.nonzero(fired.cpu().numpy())
            assert len(b) == counts[0]
            hits = sum((int(subs[i]), int(j), int(times[i])) in facts for i, j in zip(b.tolist(), y.tolist()))
            assert hits == counts[1]
            some_hits += hits
    assert some_hits > 0


def test_slab_words_past_2_31():
    """520 rules of one head x 66 001 entities x 65 words (2080 queries of that relation) are 2.23 G words per bitmap region (17.8 GB
    of scratch in one call, 2.2 GB of outputs): the slabs of the last 19 rules lie wholly beyond word 2^31 and rule 500 crosses it.  The
    graph has 160 facts with times among its first and last 20 entities, so the reference is a handful of sparse steps; the expected
    tensors are scattered on the device."""
    from red_gnn_amd import engine
    n_ent, n_rel, n_rela, trip = G.wide_graph(66001)
    n_time = 4
    rng = np.random.default_rng(12)
    base = np.column_stack([trip, rng.integers(0, n_time, len(trip))])
    ent = np.arange(n_ent)
    quads = np.concatenate([base, np.column_stack([base[:, 2], base[:, 1] + n_rel, base[:, 0], base[:, 3]]),
                            np.column_stack([ent, np.full(n_ent, n_rela - 1), ent, np.full(n_ent, n_time - 1)])], 0).astype(np.int64)
    R, B, h = 520, 2080, 1
    head, body, direc = np.full(R, h), rng.integers(0, n_rela, (R, 2)), _directions(rng, (R, 2))
    body[-1], body[-2], body[-3], body[500] = (n_rela - 1, n_rela - 1), (0, 1), (n_rela - 1, 0), (1, 3)
    direc[-1], direc[-2], direc[-3], direc[500] = (T.ANY, T.ANY), (T.ANY, T.ANY), (T.ANY, T.PAST), (T.ANY, T.ANY)
    weight = rng.integers(1, 1024, R).astype(np.float32) / np.float32(1024)
    weight[-1] = 1.0                                                             # id ^ id, the last rule, is the best of every (b, sub[b])
    pool = np.concatenate([np.arange(20), np.arange(n_ent - 20, n_ent)])
    subs = np.concatenate([pool, pool[:8], rng.integers(0, n_ent, B - 48)])
    rels, times = np.full(B, h), rng.integers(0, n_time, B)
    W = (B + 31) // 32
    assert W == 65 and 501 * n_ent * W > 2 ** 31 > 500 * n_ent * W
    budget = 20 << 30
    assert engine.rule_apply_chunking(np.full(R, n_ent * W), budget) == [(0, R)]
    g = engine.TemporalGraph(n_ent, n_rela, n_time, quads)
    cells = TA.apply_cells(n_ent, n_rela, n_time, quads, head, body, direc, weight, subs, rels, times)
    b, y, best, surv, rule, fired = A.cells_arrays(cells, n_ent)
    assert (rule >= 501).any() and (fired >= 2).any() and (rule == R - 1).any() and len(b) > B
    got = engine.trule_apply(g, head, body, direc, weight, subs, rels, times, scratch_bytes=budget)
    dev = got[0].device
    at = (torch.as_tensor(b).to(dev), torch.as_tensor(y).to(dev))
    for t, fill, vals in zip(got, (0.0, 1.0, -1, 0), (best, surv, rule, fired)):
        exp = torch.full_like(t, fill)
        exp[at] = torch.as_tensor(vals).to(dev)
        assert torch.equal(t, exp)
        del exp
    del got, g
    torch.cuda.empty_cache()                                                     # the 20 GB go back before the next test


# ---- the model entry points, on the hand graph of tests/temporal_ref.py -----------------------------------------------------------
N_BASE = 379                 # base rows of temporal_ref.hand_graph(): 253 leaf -> hub rows, 2, 120 random, 4 links; then their inverses


@pytest.fixture(scope="module")
def model_case():
    """The model of tests/test_trule_ground_gpu.py on its hand graph; a table mined with rules(k = 3) from hub -> leaf rows (inverse
    rows: a hub has about five known tails per (relation, time)) and random facts, plus one rule typed in, and its quality.

    The mined rules score the leaves of one (hub, relation, time) alike, and a tie is not moved by a filter.  The typed-in rule
    r4 ^ r0 ^ r0^-1 -> r4 tells them apart: of hub 0's r4-leaves (10, 22, 34, 46, 58 at time 2) only leaf 10 has an r0 row, the link
    (10, r0, 280, 0), so the rule reaches 10 and not its siblings; the held rows of leaves 22 and 34 then rank below the known tail
    10 unless it is filtered."""
    from red_gnn_amd.explain import TemporalRuleTable
    quads = TR.hand_graph()
    n_ent, n_rela, n_time = TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1, TR.HAND_N_TIME
    assert len(quads) == 2 * N_BASE + n_ent
    model = TR.make_model(quads, n_ent, n_rela, n_time, 3, 16, 3, "relu")
    mine = quads[np.concatenate([N_BASE + np.arange(3, 253, 11), np.arange(258, 375, 13)])]
    held = quads[np.concatenate([N_BASE + np.arange(0, 253, 7), N_BASE + np.array([19, 31]), np.arange(255, 375, 10)])]
    assert held[37].tolist() == [0, 4, 22, 2] and held[38].tolist() == [0, 4, 34, 2] and [10, 0, 280, 0] in quads.tolist()
    assert (mine[:, 1] != model.n_rel).all() and (held[:, 1] != model.n_rel).all()
    table = model.rules({"head": mine[:, 0], "relation": mine[:, 1], "time": mine[:, 3], "tail": mine[:, 2]}, k=3)
    dev = table.head.device
    one = torch.ones(1, dtype=torch.int64, device=dev)
    table = table + TemporalRuleTable(torch.tensor([4], device=dev), torch.tensor([[4, 0, 3]], device=dev),
                                      torch.full((1, 3), T.ANY, device=dev), one, one.clone(), model.n_rel)
    quality = model.rule_quality(table)
    return dict(model=model, quads=quads, n_ent=n_ent, n_rela=n_rela, n_time=n_time, mine=mine, held=held, table=table, quality=quality,
                args=(n_ent, n_rela, n_time, quads))


def _ref_weights(m, table, by_pca=False, laplace=0.0, min_hits=1, drop_trivial=True):
    """(rows kept, their weights, the rules as numpy) of rule_scores restated from the reference counts."""
    head, body, direc = (x.cpu().numpy() for x in (table.head, table.body, table.direction))
    c = T.counts(m["n_ent"], m["n_rela"], m["n_time"], m["quads"], head, body, direc)
    den = c[:, 2 if by_pca else 0] + float(laplace)
    w = np.where(den > 0, c[:, 1] / np.where(den > 0, den, 1.0), 0.0).astype(np.float32)
    step = body != m["n_rela"] - 1
    trivial = (step.sum(1) == 1) & ((body * step).sum(1) == head) & ((direc * step).sum(1) == 1)
    keep = (c[:, 1] >= min_hits) & (w > 0)
    if drop_trivial:
        keep &= ~trivial
    rows = np.nonzero(keep)[0]
    return rows, w[rows], (head[rows], body[rows], direc[rows]), trivial


def _ref_scores(m, table, q, **kw):
    rows, w, rules, _ = _ref_weights(m, table, **kw)
    ref = A.cells_to_dense(TA.apply_cells(*m["args"], *rules, w, q[:, 0], q[:, 1], q[:, 3]), len(q), m["n_ent"])
    rule = np.where(ref[2] >= 0, rows[np.maximum(ref[2], 0)], -1).astype(np.int32)
    return rows, (ref[0], ref[1], rule, ref[3])


def test_model_rule_scores_and_predict(model_case):
    from red_gnn_amd.explain import RulePrediction, RuleScores, TemporalRuleTable
    from red_gnn_amd.prediction import temporal_known_index
    m = model_case
    model, table, quality, q = m["model"], m["table"], m["quality"], m["held"]
    batch = {"head": q[:, 0], "relation": q[:, 1], "time": q[:, 3]}
    known = temporal_known_index(m["quads"], m["n_rela"], m["n_time"])
    keys, ptr, idx = known
    trivial = _ref_weights(m, table)[3]
    assert trivial.any() and np.array_equal(quality.trivial().cpu().numpy(), trivial)
    for kw, ref_kw in ((dict(), dict()), (dict(by="pca_confidence", laplace=2.0, min_hits=2, drop_trivial=False),
                                          dict(by_pca=True, laplace=2.0, min_hits=2, drop_trivial=False))):
        rows, ref = _ref_scores(m, table, q, **ref_kw)
        assert 0 < len(rows) <= table.head.numel() and (ref_kw or len(rows) < table.head.numel())
        rs = model.rule_scores(quality, batch, **kw)
        assert isinstance(rs, RuleScores) and np.array_equal(rs.rows.cpu().numpy(), rows)
        _check_types((rs.best, rs.surv, rs.best_rule, rs.fired), len(q), m["n_ent"])
        assert A.same(_np((rs.best, rs.surv, rs.best_rule, rs.fired)), ref)
        assert np.array_equal(rs.covered().cpu().numpy(), ref[3] > 0) and (ref[3] > 0).any() and (ref[3] >= 2).any()
        small = model.rule_scores(quality, batch, scratch_bytes=0, **kw)
        assert all(torch.equal(getattr(rs, f), getattr(small, f)) for f in ("best", "surv", "best_rule", "fired"))
        for agg, kn in (("noisy_or", known), ("max", known), ("noisy_or", None)):
            k = 7
            pred = model.rule_predict(quality, batch, k=k, agg=agg, known=kn, **kw)
            assert isinstance(pred, RulePrediction) and pred.table is table and isinstance(pred.table, TemporalRuleTable)
            assert [t.dtype for t in (pred.ids, pred.scores, pred.rule, pred.fired)] == [torch.int64, torch.float32, torch.int64, torch.int32]
            assert all(t.shape == (len(q), k) and t.is_cuda for t in (pred.ids, pred.scores, pred.rule, pred.fired))
            sc = A.scores(ref[0], ref[1], agg)
            dropped = 0
            for b in range(len(q)):
                key = (q[b, 0] * m["n_rela"] + q[b, 1]) * m["n_time"] + q[b, 3]
                at = np.searchsorted(keys, key)
                drop = idx[ptr[at]:ptr[at + 1]] if kn is not None and at < len(keys) and keys[at] == key else []
                dropped += len(drop)
                top = A.order(sc[b], drop)[:k]
                assert np.array_equal(pred.ids[b].cpu().numpy(), top)
                assert np.array_equal(pred.scores[b].cpu().numpy().view(np.int32), sc[b, top].view(np.int32))
                assert np.array_equal(pred.rule[b].cpu().numpy(), ref[2][b, top])
                assert np.array_equal(pred.fired[b].cpu().numpy(), ref[3][b, top])
            assert dropped >= len(q) or kn is None                               # every held row is a fact: its own tail is known
            assert len(pred.format()) == len(q) * k
    lines = model.rule_predict(quality, batch, k=3).format(id2rel=["rel%d" % i for i in range(m["n_rela"])])
    assert all(ln.startswith("row ") for ln in lines) and any("rel" in ln and "->" in ln for ln in lines)
    assert any(tag in ln for ln in lines for tag in ("[past]", "[now]", "[future]"))
    # past the end: with k = n_ent and the known tails left out, the last places are -1 / -inf / -1 / 0
    pred = model.rule_predict(quality, batch, k=m["n_ent"], known=known)
    ids = pred.ids.cpu().numpy()
    past = ids < 0
    assert (ids[:, -1] == -1).all() and (past.sum(1) >= 1).all()
    assert np.isneginf(pred.scores.cpu().numpy()[past]).all() and (pred.rule.cpu().numpy()[past] == -1).all()
    assert (pred.fired.cpu().numpy()[past] == 0).all()
    # a batch without rows
    none = model.rule_predict(quality, {"head": q[:0, 0], "relation": q[:0, 1], "time": q[:0, 3]}, k=4)
    assert all(t.shape == (0, 4) and t.is_cuda for t in (none.ids, none.scores, none.rule, none.fired))
    assert model.rule_scores(quality, {"head": q[:0, 0], "relation": q[:0, 1], "time": q[:0, 3]}).best.shape == (0, m["n_ent"])


def _filter_sets(m, q, index, with_time):
    """Per row of q the sorted union of its tail and the tails ``index`` lists for its key, as CSR int32 arrays."""
    lists = []
    for h, r, t, tau in q.tolist():
        key = (h * m["n_rela"] + r) * m["n_time"] + tau if with_time else h * m["n_rela"] + r
        mine = {t}
        if index is not None:
            at = np.searchsorted(index[0], key)
            if at < len(index[0]) and index[0][at] == key:
                mine |= set(index[2][index[1][at]:index[1][at + 1]].tolist())
        lists.append(sorted(mine))
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), np.concatenate(lists).astype(np.int32)


def _ref_metrics(m, quality, q, agg, known, known_static):
    rows, ref = _ref_scores(m, quality.table, q)
    sc = A.scores(ref[0], ref[1], agg)
    n = len(q)
    ap, ai = np.arange(n + 1, dtype=np.int32), q[:, 2].astype(np.int32)
    out = {"n": n, "coverage": float((ref[3][np.arange(n), q[:, 2]] > 0).sum()) / n}
    ranks = {}
    for sfx, index, with_time in (("", None, False), ("_fil_t", known, True), ("_fil", known_static, False)):
        fp, fi = _filter_sets(m, q, index, with_time)
        rank = rank_ref.ranks(sc, ap, ai, fp, fi)
        ranks[sfx] = rank
        out["hits1" + sfx], out["hits3" + sfx], out["hits10" + sfx] = (float(np.sum(rank <= c) / n) for c in (1, 3, 10))
        out["mrr" + sfx], out["mr" + sfx] = float(np.sum(1.0 / rank) / n), float(np.sum(rank) / n)
    return out, ranks, ref[3][np.arange(n), q[:, 2]] > 0


def test_rule_evaluate(model_case):
    from red_gnn_amd.prediction import temporal_known_index, temporal_static_known_index
    m = model_case
    model, quality, q = m["model"], m["quality"], m["held"]
    known = temporal_known_index(m["quads"], m["n_rela"], m["n_time"])
    known_static = temporal_static_known_index(m["quads"], m["n_rela"])
    for agg in ("noisy_or", "max"):
        ref, ranks, covered = _ref_metrics(m, quality, q, agg, known, known_static)
        assert 0 < ref["coverage"] <= 1
        print(agg, "ranks raw / fil_t / fil of the held rows 37, 38:", [ranks[k][37:39].tolist() for k in ("", "_fil_t", "_fil")])
        if agg == "noisy_or":                                                            # covered tails the filters move up (under "max" the
            assert covered[37] and ranks["_fil_t"][37] < ranks[""][37] and ranks["_fil"][37] < ranks[""][37]     # typed-in rule's small
            assert (covered & (ranks["_fil"] < ranks[""])).sum() >= 2                    # weight need not be a leaf's best)
        for batch_size in (256, 11):
            out = model.rule_evaluate(q, quality, agg=agg, known=known, known_static=known_static, batch_size=batch_size)
            assert set(out) == set(ref) and len(out) == 17
            assert out == ref, (agg, batch_size)
        dev = model.rule_evaluate(q, quality, agg=agg, known=tuple(torch.as_tensor(x).cuda() for x in known), known_static=known_static)
        assert dev == ref
        raw = model.rule_evaluate(torch.as_tensor(q), quality, agg=agg)                  # no index: the three ranks coincide
        assert all(raw[k] == raw[k + "_fil"] == raw[k + "_fil_t"] == ref[k] for k in ("hits1", "hits3", "hits10", "mrr", "mr"))
    # mine= is rules_all -> rule_quality -> rule_evaluate(quality=...)
    by_hand = model.rule_quality(model.rules_all(m["mine"], k=2))
    a = model.rule_evaluate(q, mine=m["mine"], k=2, known=known, known_static=known_static, laplace=1.0)
    b = model.rule_evaluate(q, quality=by_hand, known=known, known_static=known_static, laplace=1.0)
    assert a == b and a["coverage"] > 0 and a["n"] == len(q)


def test_model_errors(model_case):
    from red_gnn_amd.explain import RuleQuality, RuleTable, TemporalRuleQuality, TemporalRuleTable
    m = model_case
    model, quality, t, q = m["model"], m["quality"], m["table"], m["held"][:4]
    batch = {"head": q[:, 0], "relation": q[:, 1], "time": q[:, 3]}
    static = RuleQuality(RuleTable(t.head, t.body, t.support, t.fixed, t.n_rel), quality.body_pairs, quality.hits, quality.pca_body_pairs,
                         quality.head_pairs, 7)
    wrong = TemporalRuleQuality(TemporalRuleTable(t.head, t.body, t.direction, t.support, t.fixed, t.n_rel + 1), quality.body_pairs,
                                quality.hits, quality.pca_body_pairs, quality.head_pairs, quality.n_anchors)
    for name, call in (("rule_scores", lambda x: model.rule_scores(x, batch)), ("rule_predict", lambda x: model.rule_predict(x, batch)),
                       ("rule_evaluate", lambda x: model.rule_evaluate(q, x))):
        for bad in (static, t, None if name != "rule_evaluate" else 5):
            with pytest.raises(ValueError, match="%s: quality must be an explain.TemporalRuleQuality" % name):
                call(bad)
        with pytest.raises(ValueError, match="%s: the table has n_rel=%d, the model n_rel=%d" % (name, t.n_rel + 1, t.n_rel)):
            call(wrong)
    with pytest.raises(ValueError, match="rule_predict: agg must be"):
        model.rule_predict(quality, batch, agg="mean")
    for k in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="rule_predict: k must be an integer in 1"):
            model.rule_predict(quality, batch, k=k)
    with pytest.raises(ValueError, match="rule_predict: known must be"):
        model.rule_predict(quality, batch, known=(1, 2))
    with pytest.raises(ValueError, match="rule_scores: the batch needs"):
        model.rule_scores(quality, {"head": q[:, 0]})
    with pytest.raises(ValueError, match="out of range"):
        model.rule_scores(quality, dict(batch, time=q[:, 3] + m["n_time"]))
    with pytest.raises(ValueError, match="rule_scores: by must be"):
        model.rule_scores(quality, batch, by="hits")
    with pytest.raises(ValueError, match="rule_evaluate: agg must be"):
        model.rule_evaluate(q, quality, agg="sum")
    for k in (0, 9, 1.5):
        with pytest.raises(ValueError, match="rule_evaluate: k must be an integer in 1"):
            model.rule_evaluate(q, mine=m["mine"], k=k)
    for bs in (0, -3, 2.5):
        with pytest.raises(ValueError, match="rule_evaluate: batch_size must be a positive integer"):
            model.rule_evaluate(q, quality, batch_size=bs)
    with pytest.raises(ValueError, match="rule_evaluate: give exactly one of quality"):
        model.rule_evaluate(q)
    with pytest.raises(ValueError, match="rule_evaluate: give exactly one of quality"):
        model.rule_evaluate(q, quality, mine=m["mine"])
    with pytest.raises(ValueError, match="rule_evaluate: quads must be"):
        model.rule_evaluate(q[:, :3], quality)
    with pytest.raises(ValueError, match="rule_evaluate: known must be"):
        model.rule_evaluate(q, quality, known=(1, 2))


# ---- the C entry point itself -----------------------------------------------------------------------------------------------------
def _raw(graph, rules, queries, q_row=None, n_rules=None, n_hops=None, n_words=None, phases=3, batch=None, rule_base=0):
    """rg_trule_apply on rules (head, body, direction, weight) and queries (subs, rels, times) laid out as engine.trule_apply lays them
    out, the ids unvalidated: the four outputs as numpy."""
    from red_gnn_amd import _lib, engine
    dev = torch.device("cuda")
    head, body, direc, weight = (np.asarray(a) for a in rules)
    subs, rels, times = (np.asarray(a, np.int64) for a in queries)
    n_ent, n_rows = graph.n_ent, getattr(graph, "n_rela_rows", 2 * graph.n_rel + 1)              # (a static graph, refused, has neither)
    n_time = max(getattr(graph, "n_time", 0), 1)
    B, R, L = len(subs), len(head), body.shape[1]
    key = rels * n_time + times
    order = np.argsort(key, kind="stable")
    q_ptr = np.searchsorted(key[order], np.arange(n_rows * n_time + 1)).astype(np.int32)
    per_rel = np.diff(q_ptr[::n_time].astype(np.int64))
    ok = (head >= 0) & (head < n_rows)
    words = np.where(ok, n_ent * ((per_rel[np.where(ok, head, 0)] + 31) // 32), 0)
    slab = np.concatenate([[0], np.cumsum(words)]).astype(np.int64)
    row = order.astype(np.int32) if q_row is None else np.asarray(q_row, np.int32)
    to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
    keep = [to(head, np.int32), to(body, np.int32), to(direc, np.int32), to(weight, np.float32), to(A.miss_of(weight), np.float32),
            to(subs[order], np.int32), to(row, np.int32), to(q_ptr, np.int32), to(slab, np.int64)]
    total = max(int(slab[-1]), 1)
    scratch = torch.empty(engine.rule_apply_scratch_bytes(total), dtype=torch.uint8, device=dev)
    out = (torch.zeros((B, n_ent), dtype=torch.float32, device=dev), torch.ones((B, n_ent), dtype=torch.float32, device=dev),
           torch.full((B, n_ent), -1, dtype=torch.int32, device=dev), torch.zeros((B, n_ent), dtype=torch.int32, device=dev))
    p = _lib.ptr
    _lib.check(_lib.lib().rg_trule_apply(graph.handle, *(p(k) for k in keep[:5]), R if n_rules is None else n_rules,
                                         L if n_hops is None else n_hops, rule_base, p(keep[5]), p(keep[6]), p(keep[7]),
                                         B if batch is None else batch, p(keep[8]), total if n_words is None else n_words, p(scratch),
                                         phases, *(p(o) for o in out), _lib.stream_ptr()))
    return _np(out)


def test_entry_point_errors(case):
    from red_gnn_amd import _lib, engine
    c = case
    tg = c["graph"]
    r = tuple(a[:1] for a in c["rules"][2])
    q = (c["subs"][:1], np.full(1, r[0][0]), c["times"][:1])
    sg = engine.Graph(5, 2, np.array([[0, 0, 1], [1, 1, 2], [3, 0, 4]]))
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: static graph .*use rg_rule_apply"):
        _raw(sg, (np.array([0]), np.array([[0, 1]]), np.array([[3, 3]]), np.ones(1, np.float32)), (np.array([0]), np.array([0]), np.array([0])))
    with pytest.raises(ValueError, match="trule_apply: static graph"):
        engine.trule_apply(sg, np.array([0]), np.array([[0, 1]]), np.array([[3, 3]]), np.ones(1, np.float32), np.array([0]), np.array([0]),
                           np.array([0]))
    # the static entry points still refuse the temporal graph
    with pytest.raises(ValueError, match="^rule_apply: temporal graph"):
        engine.rule_apply(tg, np.array([0]), np.array([[0, 1]]), np.array([0.5], np.float32), np.array([0]), np.array([0]))
    dev = torch.device("cuda")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    slab = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    scratch = torch.zeros(engine.rule_apply_scratch_bytes(3), dtype=torch.uint8, device=dev)
    out = (f32(3), f32(3), i32(3), i32(3))
    p = _lib.ptr
    with pytest.raises(_lib.NativeError, match="rg_rule_apply: temporal graph"):
        _lib.check(_lib.lib().rg_rule_apply(tg.handle, p(i32(1)), p(i32(2)), p(f32(1)), p(f32(1)), 1, 2, 0, p(i32(1)), p(i32(1)),
                                            p(i32(64)), 1, p(slab), 3, p(scratch), 3, *(p(o) for o in out), _lib.stream_ptr()))
    assert not any(o.any() for o in out)
    for hops in (0, 33):
        with pytest.raises(_lib.NativeError, match="rg_trule_apply: n_hops=%d not in 1..32" % hops):
            _raw(tg, r, q, n_hops=hops)
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: n_rules=65536 not in"):
        _raw(tg, r, q, n_rules=65536)
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: n_rules=-1 not in"):
        _raw(tg, r, q, n_rules=-1)
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: batch=-1"):
        _raw(tg, r, q, batch=-1)
    for ph in (0, 4):
        with pytest.raises(_lib.NativeError, match="rg_trule_apply: phases=%d not in 1..3" % ph):
            _raw(tg, r, q, phases=ph)
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: rule_base=-1"):
        _raw(tg, r, q, rule_base=-1)
    with pytest.raises(_lib.NativeError, match="rg_trule_apply: n_words=0 is outside"):
        _raw(tg, r, q, n_words=0)
    assert A.same(_raw(tg, r, q, n_rules=0), A.initial(1, c["n_ent"])) and A.same(_raw(tg, r, q, batch=0), A.initial(1, c["n_ent"]))
    # this file's layout of the raw call is the engine's
    pick = np.arange(0, len(c["subs"]), 9)
    qs = (c["subs"][pick], c["rels"][pick], c["times"][pick])
    assert A.same(_raw(tg, c["rules"][3], qs), tuple(a[pick] for a in c["ref"][3]))


def test_ids_are_bounded_in_the_kernel(case):
    """The C entry point trusts its caller for the ids (engine.trule_apply validates them).  Read in csrc/trule_apply.hip and
    rule_slabs.h before this was run: tapply_hop_kernel tests the step's relation and direction before rel_ptr is read and leaves,
    rule_slab() tests the head against 0..n_rela_rows-1 before q_ptr is read, and the aggregate skips a q_row outside 0..batch-1
    before it forms a cell index.  A rule whose step names relation n_rela_rows or -1, or direction 4, reaches nothing; a rule whose
    head is no relation has no slab; a sorted position whose q_row is ``batch`` writes nothing; every other cell is the reference's."""
    c = case
    pick = np.arange(0, len(c["subs"]), 6)
    subs, rels, times = c["subs"][pick], c["rels"][pick], c["times"][pick]
    B = len(subs)
    head, body, direc, weight = (a.copy() for a in c["rules"][3])
    full = A.cells_to_dense(TA.apply_cells(*c["args"], head, body, direc, weight, subs, rels, times), B, c["n_ent"])
    bad = [4, 17, 30, 44]
    body[4, 1], body[17, 0], direc[30, 2] = c["n_rela"], -1, 4
    head[-1] = 2 ** 31 - 1                                                     # sorted still: the largest head
    bad.append(len(head) - 1)
    good = np.setdiff1d(np.arange(len(head)), bad)
    # the reference of the good rules alone, under their indices in the whole list
    cells = {}
    for i in good.tolist():
        cells = TA.apply_cells(*c["args"], head[i:i + 1], body[i:i + 1], direc[i:i + 1], weight[i:i + 1], subs, rels, times, state=cells,
                               rule_base=i)
    ref = A.cells_to_dense(cells, B, c["n_ent"])
    assert not A.same(ref, full) and (ref[3] > 0).any()                        # the rules made bad did fire before
    got = _raw(c["graph"], (head, body, direc, weight), (subs, rels, times))
    assert A.same(got, ref)
    # one query's row index is `batch`: that row stays at its initial values, the others do not change
    key = rels * c["n_time"] + times
    order = np.argsort(key, kind="stable").astype(np.int32)
    lost = int(np.nonzero(ref[3].sum(1) > 0)[0][0])
    row = order.copy()
    row[order == lost] = B
    got = _raw(c["graph"], (head, body, direc, weight), (subs, rels, times), q_row=row)
    exp = tuple(a.copy() for a in ref)
    for a, init in zip(exp, A.initial(1, c["n_ent"])):
        a[lost] = init[0]
    assert A.same(got, exp)
