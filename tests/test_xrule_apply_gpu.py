"""engine.xrule_apply (rg_xrule_apply, csrc/xrule_apply.hip) and extrapolation.T_RED_GNN.rule_scores / rule_predict / rule_evaluate on
the MI355X (-m gpu): every output equal bit for bit to tests/xrule_apply_ref.py on the data the device graph was built from - the hand
data set with its typed-in cells, the 150-entity fixture of tests/test_xrule_ground_gpu.py under 40 random rules of every bin with one
relation of more words than a wave and query days with empty windows, with windows from row 0 and with gaps between them, per-relation
query counts around the word boundaries, the smallest chunking, a raw two-call split, the phases apart, other path lengths, the counts
of rg_xrule_ground, the model entry points, the errors, and the kernel's own bounds on its ids and layout arrays."""
import numpy as np
import pytest
import torch

from tests import extrap_ref as ER
from tests import rank_ref
from tests import rule_apply_ref as A
from tests import xrule_apply_ref as XA
from tests import xrule_ground_ref as X

pytestmark = pytest.mark.gpu

BOUNDARY_COUNTS = (1, 31, 32, 33, 64, 65)
# query days: 1, 52 and 121 have empty windows (no row on the day before), 171 and 172 windows from row 0 with lags above 120, 170 a
# full window whose first row has lag 121; the others lie between them, and the days not listed hold no query
QUERY_DAYS = np.array([1, 20, 52, 60, 61, 100, 121, 150, 170, 171, 172, 200, 219])
BIG, BIG_N, ONE_DAY, ONE_DAY_N = 2, 2112, 4, 33          # relation 2 has 2112 queries = 66 words; relation 4 has 33, all on day 171


# stated from the reference alone (build_case on the host): 40 rules, 2350 queries x 150 entities
MIN_FIRING_RULES = 25
MIN_CELLS_FIRED_TWICE = 1500


def _np(four):
    return tuple(t.cpu().numpy() for t in four)


def _check_types(four, B, n_ent):
    assert all(t.is_cuda and t.shape == (B, n_ent) for t in four)
    assert [t.dtype for t in four] == [torch.float32, torch.float32, torch.int32, torch.int32]


def _weights(rng, n):
    return rng.integers(1, 257, n).astype(np.float32) / np.float32(256)


def _sorted_rules(rng, r):
    """(head, body, lag_lo, lag_hi, weight) of random_rules' (head, body, lag_lo, lag_hi), stably sorted by head, with random weights."""
    return XA.sort_by_head(*r)[1:] + (_weights(rng, len(r[0])),)


def _hand_graph():
    from red_gnn_amd import engine
    return engine.TemporalGraph(X.HAND_N_ENT, X.HAND_N_REL + 1, len(X.HAND_DATA) + 1, X.graph_rows(X.HAND_DATA, X.HAND_N_ENT, X.HAND_N_REL))


def test_hand_data_set():
    from red_gnn_amd import engine
    g = _hand_graph()
    lo, hi = X.windows(X.HAND_OFF)
    data = (X.HAND_N_ENT, X.HAND_N_REL, X.HAND_DATA, X.HAND_ROW_DAY, lo, hi)
    rules, q = XA.hand_rules() + (XA.HAND_WEIGHT,), XA.HAND_QUERIES
    B = len(q)
    apply = lambda r, s, p, t, **kw: engine.xrule_apply(g, *r, s, p, t, X.HAND_ROW_DAY, lo, hi, **kw)
    got = apply(rules, q[:, 0], q[:, 1], q[:, 2])
    _check_types(got, B, X.HAND_N_ENT)
    assert XA.same(_np(got), XA.hand_expected())                                                  # the typed-in cells
    assert XA.same(_np(got), XA.apply_dense(*data, *rules, q[:, 0], q[:, 1], q[:, 2]))
    fired = _np(got)[3]
    assert sorted((b, y) for b, y in np.argwhere(fired).tolist()) == sorted({c for cells in XA.HAND_FIRING for c in cells})
    assert fired[0, 2] == 2 and fired[4, 1] == 2 and not fired[6].any() and not fired[9].any()
    as_t = lambda a: torch.as_tensor(a).cuda()
    again = engine.xrule_apply(g, *(as_t(a) for a in rules), *(as_t(q[:, c]) for c in range(3)), as_t(X.HAND_ROW_DAY), as_t(lo), as_t(hi))
    assert XA.same(_np(again), XA.hand_expected())
    # the 12 default anchors as queries under each rule's head: the cells a rule fires for are its body pairs
    a = X.HAND_ANCHORS
    for i in range(7):
        one = tuple(x[i:i + 1] for x in rules)
        f = _np(apply(one, a[:, 0], np.full(len(a), one[0][0]), a[:, 1]))[3]
        assert int(f.sum()) == XA.HAND_BODY_PAIRS[i] == X.HAND_ALL[XA.HAND_ORDER[i], 0], i
    # a self-loop's lag is min(t, loop_window): id[4-7d] -> r1 fires for q0 (day 4) alone, and with loop_window = 4 for the r1 queries
    # of days 122 and 123 too (q1, q2, q7; q8 is of day 0)
    loop = (np.array([1]), np.array([[3]]), np.array([[4]]), np.array([[8]]), np.array([0.5], np.float32))
    for lw, n in ((120, 1), (4, 4), (0, 0)):
        f = _np(apply(loop, q[:, 0], q[:, 1], q[:, 2], loop_window=lw))
        assert XA.same(f, XA.apply_dense(*data, *loop, q[:, 0], q[:, 1], q[:, 2], loop_window=lw)) and f[3].sum() == n, lw
    none = apply(tuple(x[:0] for x in rules), q[:, 0], q[:, 1], q[:, 2])                           # R = 0
    _check_types(none, B, X.HAND_N_ENT)
    assert XA.same(_np(none), A.initial(B, X.HAND_N_ENT))
    _check_types(apply(rules, q[:0, 0], q[:0, 1], q[:0, 2]), 0, X.HAND_N_ENT)                      # B = 0
    only = apply(rules, np.array([2]), np.array([2]), np.array([4]))                               # no rule has a query
    assert XA.same(_np(only), A.initial(1, X.HAND_N_ENT))


def build_case(data):
    """What the fixture holds beside the model, formed on the host: the windows, 40 random rules (L = 1, 2, 3; every bin, ANY and
    identity steps) sorted by head with random weights, the queries and the reference outputs, computed once."""
    n_ent, n_rel = ER.N_ENT, ER.N_REL
    row_day = data[:, 3] // 24
    off = X.offsets(row_day)
    lo, hi = X.windows(off)
    n_day = len(off)
    rng = np.random.default_rng(29)
    rules = {L: _sorted_rules(rng, r) for L, r in X.random_rules(np.random.default_rng(17), 40, n_rel + 1).items()}
    counts = {0: 70, 1: 40, BIG: BIG_N, 3: 31, ONE_DAY: ONE_DAY_N, 5: 64}
    rels = np.concatenate([np.full(n, r) for r, n in counts.items()])
    B = len(rels)
    subs, days = rng.integers(0, n_ent, B), rng.choice(QUERY_DAYS, B)
    days[rels == ONE_DAY] = 171
    mix = rng.permutation(B)
    subs, rels, days = subs[mix], rels[mix], days[mix]
    twin = np.nonzero(rels == BIG)[0][:2]                                       # a query stated twice
    subs[twin[1]], days[twin[1]] = subs[twin[0]], days[twin[0]]
    base = (n_ent, n_rel, data, row_day, lo, hi)
    ref = {L: XA.apply_lists(*base, *r, subs, rels, days) for L, r in rules.items()}
    fire = XA.firing_lists(*base, subs, rels, days)
    n_fire = {L: [len(fire(*rule)[0]) for rule in zip(*(np.asarray(x).tolist() for x in r[:4]))] for L, r in rules.items()}
    return dict(data=data, n_ent=n_ent, n_rel=n_rel, n_day=n_day, row_day=row_day, off=off, lo=lo, hi=hi, base=base, rules=rules, subs=subs,
                rels=rels, days=days, ref=ref, n_fire=n_fire, default=X.default_anchors(data, row_day, n_ent))


@pytest.fixture(scope="module")
def case():
    """extrap_ref.make_case(32, 9) + make_model, the fixture of tests/test_xrule_ground_gpu.py: 150 entities, 6 relations + the
    identity, 6000 rows over 220 days; the graph, row days and offsets are the model's own.  build_case(): the rules, 2350 queries
    and the reference."""
    from red_gnn_amd import engine
    data, queries = ER.make_case(32, 9)
    model = ER.make_model(data, 32, 5, "tanh", 3)
    c = build_case(data)
    assert model.n_rel_true == c["n_rel"] and model.graph.n_rela_rows == c["n_rel"] + 2 and model.graph.n_time == len(data) + 1
    assert np.array_equal(model.row_time.cpu().numpy(), c["row_day"]) and np.array_equal(model.time_offset_list, c["off"])
    assert np.array_equal(model.windows()[0], c["lo"]) and np.array_equal(model.windows()[1], c["hi"])

    def apply(r, subs, rels, days, **kw):
        got = engine.xrule_apply(model.graph, *r, subs, rels, days, c["row_day"], c["lo"], c["hi"], **kw)
        _check_types(got, len(subs), c["n_ent"])
        return _np(got)
    c.update(model=model, graph=model.graph, queries=queries, apply=apply,
             ref_of=lambda r, subs, rels, days, **kw: XA.apply_lists(*c["base"], *r, subs, rels, days, **kw))
    return c


def test_the_queries_are_the_ones_described(case):
    c = case
    rels, days, lo, hi = c["rels"], c["days"], c["lo"], c["hi"]
    assert ((rels == BIG).sum() + 31) // 32 == 66 and (rels == ONE_DAY).sum() == 33 and set(days[rels == ONE_DAY].tolist()) == {171}
    assert set(days[rels == BIG].tolist()) == set(QUERY_DAYS.tolist())                       # every listed day, and gaps between them
    assert all(lo[t] >= hi[t] for t in (1, 52, 121))                                         # empty windows
    assert all(lo[t] == 0 and hi[t] > 0 and t - c["row_day"][0] > 120 for t in (171, 172))   # from row 0: lags above 120
    assert lo[170] > 0 and 170 - c["row_day"][lo[170]] == 121
    body = np.concatenate([r[1].reshape(-1) for r in c["rules"].values()])
    lag_lo = np.concatenate([r[2].reshape(-1) for r in c["rules"].values()])
    lag_hi = np.concatenate([r[3].reshape(-1) for r in c["rules"].values()])
    assert len(body) == 14 * 1 + 13 * 2 + 13 * 3 and (body == c["n_rel"]).any()
    assert set(lag_lo.tolist()) == {0, 2, 4, 8, 15, 31, 61, 121} and ((lag_lo == 0) & (lag_hi == X.ANY_HI)).any()      # every bin, and ANY
    assert all((np.diff(r[0]) >= 0).all() for r in c["rules"].values())


def test_random_rules_equal_the_reference(case):
    c = case
    firing, twice, old = 0, 0, 0
    for L, r in c["rules"].items():
        got = c["apply"](r, c["subs"], c["rels"], c["days"])
        assert XA.same(got, c["ref"][L]), L
        firing += sum(n > 0 for n in c["n_fire"][L])
        twice += int((c["ref"][L][3] >= 2).sum())
        step_old = (r[2] == 121) & (r[1] != c["n_rel"])                          # a data-row step in the open last bin ...
        old += sum(n for n, o in zip(c["n_fire"][L], step_old.any(1)) if o)      # ... fires: days 171 and 172 see lags above 120
    assert firing >= MIN_FIRING_RULES and twice >= MIN_CELLS_FIRED_TWICE and old > 0          # not a comparison of zeros
    # the definition itself on a part of the queries (the dense form is slow beyond a few days)
    part = np.nonzero(np.isin(c["days"], [20, 52, 121, 171]) & np.isin(c["rels"], [0, 1, 3, ONE_DAY]))[0]
    assert len(part) >= 40
    r, q = c["rules"][2], (c["subs"][part], c["rels"][part], c["days"][part])
    dense = XA.apply_dense(*c["base"], *r, *q)
    assert XA.same(c["apply"](r, *q), dense) and (dense[3] > 0).any()


@pytest.mark.parametrize("n", BOUNDARY_COUNTS)
def test_query_counts_around_the_word_boundaries(case, n):
    """n queries of every relation: W = 1, 1, 1, 2, 2, 3 words, the last word full, one bit short or one bit long."""
    c = case
    rng = np.random.default_rng(300 + n)
    rels = np.repeat(np.arange(c["n_rel"]), n)
    subs, days = rng.integers(0, c["n_ent"], len(rels)), rng.choice(QUERY_DAYS, len(rels))
    mix = rng.permutation(len(rels))
    q = (subs[mix], rels[mix], days[mix])
    some = 0
    for L, r in c["rules"].items():
        got = c["apply"](r, *q)
        assert XA.same(got, c["ref_of"](r, *q)), L
        some += int(got[3].sum())
    assert some > 0


def test_day_ranges_on_word_boundaries(case):
    """Every entry's columns start and end on a word boundary: 32 queries a day on three days, 64 on one."""
    c = case
    rng = np.random.default_rng(8)
    for days in ([60, 61, 172], [171, 171]):
        d = np.repeat(days, 32)
        q = (rng.integers(0, c["n_ent"], len(d)), np.full(len(d), BIG), d)
        for L, r in c["rules"].items():
            got = c["apply"](r, *q)
            assert XA.same(got, c["ref_of"](r, *q)), (days, L)


def test_chunking_changes_no_bit(case):
    from red_gnn_amd import engine
    c = case
    q = (c["subs"], c["rels"], c["days"])
    for L, r in c["rules"].items():
        events = engine.XRULE_APPLY_EVENTS = []
        try:
            small = c["apply"](r, *q, scratch_bytes=0)                            # the smallest budget: one rule per call
        finally:
            engine.XRULE_APPLY_EVENTS = None
        assert XA.same(small, c["ref"][L]), L
        assert len(events) == len(r[0]) and {e[3] for e in events} == {1}         # every head relation has queries
        words = c["n_ent"] * ((np.bincount(c["rels"], minlength=8)[r[0]] + 31) // 32)
        assert [e[4] for e in events] == words.tolist()
    r = c["rules"][3]
    mid = engine.rule_apply_scratch_bytes(c["n_ent"] * (66 + 3))                  # a few rules per call
    assert XA.same(c["apply"](r, *q, scratch_bytes=mid), c["ref"][3])


@pytest.mark.parametrize("L", [1, 4])
def test_other_path_lengths(case, L):
    c = case
    rng = np.random.default_rng(200 + L)
    bins = np.where(rng.integers(0, 2, (20, L)) == 0, 8, rng.integers(0, 8, (20, L)))
    r = _sorted_rules(rng, (rng.integers(0, c["n_rel"], 20), rng.integers(0, c["n_rel"] + 1, (20, L))) + X.bin_ranges(bins))
    pick = np.arange(0, len(c["subs"]), 3)
    q = (c["subs"][pick], c["rels"][pick], c["days"][pick])
    got = c["apply"](r, *q)
    assert XA.same(got, c["ref_of"](r, *q)) and (got[3] > 0).any()


def test_agrees_with_the_grounding_kernel(case):
    """Per rule, the cells it fires for with the default anchors as queries under its head are its body_pairs of rg_xrule_ground."""
    from red_gnn_amd import engine
    c = case
    a = c["default"]
    assert len(a) == 4062
    total = 0
    for L, r in c["rules"].items():
        counts = engine.xrule_ground(c["graph"], r[0], r[1], r[2], r[3], c["row_day"], c["lo"], c["hi"]).cpu().numpy()
        for i in range(len(r[0])):
            one = tuple(x[i:i + 1] for x in r)
            fired = c["apply"](one, a[:, 0], np.full(len(a), r[0][i]), a[:, 1])[3]
            assert int(fired.sum()) == counts[i, 0] and fired.max() <= 1, (L, i)
            total += int(counts[i, 0])
    assert total > 0


# ---- the C entry point itself -----------------------------------------------------------------------------------------------------
class Raw:
    """rg_xrule_apply on rules (head, body, lag_lo, lag_hi, weight) and queries (subs, rels, days) laid out as engine.xrule_apply lays
    them out (engine.xrule_query_layout, clipped ids for the layout only), the ids unvalidated.  The arrays are numpy attributes a test
    may overwrite before call(); the outputs and the scratch persist between calls."""

    def __init__(self, c, graph, rules, queries, n_words=None):
        from red_gnn_amd import engine
        self.c, self.graph = c, graph
        self.head, self.body, self.lag_lo, self.lag_hi, self.weight = (np.asarray(a).copy() for a in rules)
        subs, rels, days = (np.asarray(a, np.int64) for a in queries)
        self.n_ent, self.n_rows = graph.n_ent, getattr(graph, "n_rela_rows", 0) or 8
        order, self.q_ptr, self.day_ptr, self.day_of, self.day_pos = engine.xrule_query_layout(rels, days, self.n_rows, c["n_day"])
        self.q_sub, self.q_row, self.B = subs[order], order.astype(np.int32), len(subs)
        self.row_day, self.win_lo, self.win_hi = c["row_day"], c["lo"], c["hi"]
        self.slab = self.slabs(self.head)
        dev = torch.device("cuda")
        self.total = max(int(self.slab[-1]), 1) if n_words is None else n_words
        self.scratch = torch.empty(max(engine.rule_apply_scratch_bytes(max(int(self.slab[-1]), 1)), 256), dtype=torch.uint8, device=dev)
        self.out = (torch.zeros((self.B, self.n_ent), dtype=torch.float32, device=dev),
                    torch.ones((self.B, self.n_ent), dtype=torch.float32, device=dev),
                    torch.full((self.B, self.n_ent), -1, dtype=torch.int32, device=dev),
                    torch.zeros((self.B, self.n_ent), dtype=torch.int32, device=dev))

    def slabs(self, head):
        per_rel = np.diff(self.q_ptr.astype(np.int64))
        ok = (head >= 0) & (head < self.n_rows)
        words = np.where(ok, self.n_ent * ((per_rel[np.where(ok, head, 0)] + 31) // 32), 0)
        return np.concatenate([[0], np.cumsum(words)]).astype(np.int64)

    def call(self, r0=0, r1=None, phases=3, n_rules=None, n_hops=None, batch=None, rule_base=None, n_data=None, n_day=None,
             loop_window=120, n_qdays=None, null=()):
        """The rules r0..r1 (their own slabs, rule_base = r0) on the persistent outputs; ``null``: argument names passed as NULL."""
        from red_gnn_amd import _lib
        dev = torch.device("cuda")
        r1 = len(self.head) if r1 is None else r1
        to = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(dev)
        slab = self.slab[r0:r1 + 1] - self.slab[r0]
        t = dict(head=to(self.head[r0:r1], np.int32), body=to(self.body[r0:r1], np.int32), lag_lo=to(self.lag_lo[r0:r1], np.int32),
                 lag_hi=to(self.lag_hi[r0:r1], np.int32), weight=to(self.weight[r0:r1], np.float32),
                 miss=to(A.miss_of(self.weight[r0:r1]), np.float32), row_day=to(self.row_day, np.int32), win_lo=to(self.win_lo, np.int32),
                 win_hi=to(self.win_hi, np.int32), q_sub=to(self.q_sub, np.int32), q_row=to(self.q_row, np.int32),
                 q_ptr=to(self.q_ptr, np.int32), day_ptr=to(self.day_ptr, np.int32), day_of=to(self.day_of, np.int32),
                 day_pos=to(self.day_pos, np.int32), slab=to(slab, np.int64), scratch=self.scratch)
        p = lambda k: None if k in null else _lib.ptr(t[k])
        o = [None if "best" in null and k == 0 else _lib.ptr(x) for k, x in enumerate(self.out)]
        total = self.total if (r0, r1) == (0, len(self.head)) else max(int(slab[-1]), 1)
        _lib.check(_lib.lib().rg_xrule_apply(
            self.graph.handle, p("head"), p("body"), p("lag_lo"), p("lag_hi"), p("weight"), p("miss"), r1 - r0 if n_rules is None else n_rules,
            self.body.shape[1] if n_hops is None else n_hops, r0 if rule_base is None else rule_base, p("row_day"),
            len(self.row_day) if n_data is None else n_data, p("win_lo"), p("win_hi"), self.c["n_day"] if n_day is None else n_day, loop_window,
            p("q_sub"), p("q_row"), p("q_ptr"), p("day_ptr"), p("day_of"), p("day_pos"), len(self.day_of) if n_qdays is None else n_qdays,
            self.B if batch is None else batch, p("slab"), total, p("scratch"), phases, *o, _lib.stream_ptr()))
        return _np(self.out)


def _part(c, step=7):
    pick = np.arange(0, len(c["subs"]), step)
    return c["subs"][pick], c["rels"][pick], c["days"][pick]


def test_raw_call_split_and_phases(case):
    c = case
    q = _part(c, 5)
    for L, r in c["rules"].items():
        ref = c["ref_of"](r, *q)
        assert XA.same(Raw(c, c["graph"], r, q).call(), ref), L                  # this file's layout of the raw call is the engine's
        # two calls with rule_base, the outputs carried: against the reference with ``state``
        cut = len(r[0]) // 2
        first = c["ref_of"](tuple(x[:cut] for x in r), *q)
        two = Raw(c, c["graph"], r, q)
        assert XA.same(two.call(0, cut), first) and not XA.same(first, ref)
        assert XA.same(two.call(cut, None), c["ref_of"](tuple(x[cut:] for x in r), *q, state=first, rule_base=cut))
        assert XA.same(_np(two.out), ref)
        # phase 1 leaves the bitmaps in the scratch and the outputs alone, phase 2 folds them
        apart = Raw(c, c["graph"], r, q)
        assert XA.same(apart.call(phases=1), A.initial(len(q[0]), c["n_ent"]))
        assert XA.same(apart.call(phases=2), ref)


def test_entry_point_errors(case):
    from red_gnn_amd import _lib, engine
    c = case
    xg = c["graph"]
    r = tuple(x[:1] for x in c["rules"][2])
    q = (c["subs"][:1], np.full(1, r[0][0]), c["days"][:1])

    def raw(g=xg, n_words=None, **kw):
        return Raw(c, g, r, q, n_words=n_words).call(**kw)
    sg = engine.Graph(5, 2, np.array([[0, 0, 1], [1, 1, 2], [3, 0, 4]]))
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: not the extrapolation layout"):
        raw(sg)
    tg = engine.TemporalGraph(5, 3, 4, np.array([[0, 0, 1, 0], [1, 1, 2, 3], [3, 2, 3, 3]]))      # an interpolation graph: 4 time ids
    with pytest.raises(_lib.NativeError, match=r"rg_xrule_apply: not the extrapolation layout \(n_time=4, n_data=6000"):
        raw(tg)
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: not the extrapolation layout"):
        raw(n_data=5999)
    with pytest.raises(ValueError, match="xrule_apply: not the extrapolation layout"):
        engine.xrule_apply(tg, *r, *q, c["row_day"], c["lo"], c["hi"])
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: NULL graph"):
        _lib.check(_lib.lib().rg_xrule_apply(*([None] * 7), 1, 1, 0, None, 6000, None, None, 1, 120, *([None] * 6), 1, 1, None, 1, None, 3,
                                             *([None] * 5)))
    for name in ("head", "lag_hi", "miss", "row_day", "win_lo", "q_row", "day_ptr", "day_of", "day_pos", "slab", "scratch", "best"):
        with pytest.raises(_lib.NativeError, match="rg_xrule_apply: NULL argument"):
            raw(null=(name,))
    for hops in (0, 33):
        with pytest.raises(_lib.NativeError, match="rg_xrule_apply: n_hops=%d not in 1..32" % hops):
            raw(n_hops=hops)
    for n in (65536, -1):
        with pytest.raises(_lib.NativeError, match="rg_xrule_apply: n_rules=%d not in" % n):
            raw(n_rules=n)
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: batch=-1"):
        raw(batch=-1)
    for ph in (0, 4):
        with pytest.raises(_lib.NativeError, match="rg_xrule_apply: phases=%d not in 1..3" % ph):
            raw(phases=ph)
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: rule_base=-1"):
        raw(rule_base=-1)
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: n_day=0"):
        raw(n_day=0)
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: loop_window=-1"):
        raw(loop_window=-1)
    with pytest.raises(_lib.NativeError, match="rg_xrule_apply: n_qdays=-1"):
        raw(n_qdays=-1)
    for words in (0, -5, (1 << 40) + 1):
        with pytest.raises(_lib.NativeError, match="rg_xrule_apply: n_words=%d is outside" % words):
            raw(n_words=words)
    init = A.initial(1, c["n_ent"])
    assert XA.same(raw(n_rules=0), init) and XA.same(raw(batch=0), init)
    assert XA.same(raw(n_qdays=0), init)                                          # no entry: every rule leaves
    assert XA.same(raw(), c["ref_of"](r, *q))


def test_ids_and_layout_are_bounded_in_the_kernel(case):
    """The C entry point trusts its caller for the ids and the query layout (engine.xrule_apply forms and validates them).  Read in
    csrc/xrule_apply.hip and rule_slabs.h before this was run: xapply_hop_kernel tests the step's relation and its lag range before
    rel_ptr is read; rule_slab() tests the head against 0..n_rela_rows-1 before q_ptr or day_ptr is read and the slab against
    0..n_words; day_ptr is clamped to 0..n_qdays before day_of or day_pos is indexed, both binary searches stay inside those bounds
    whatever day_of holds, a day_of value is tested against 0..n_day-1 before it indexes a window, day_pos and q_ptr values are clamped
    to 0..batch and every range to 0..S_i before move_range; edge ends, row indices and row days are tested as in xrule_ground.hip; the
    aggregate skips a q_row outside 0..batch-1 before it forms a cell index.  So: a rule made bad reaches nothing or something
    unspecified, and every cell of the other rules is the reference's."""
    c = case
    q = _part(c, 4)
    B = len(q[0])
    r = tuple(x.copy() for x in c["rules"][3])
    head, body, lo, hi, weight = r
    n_rela = c["graph"].n_rela_rows
    full = c["ref_of"](r, *q)

    def ref_without(bad):
        state = None
        for i in np.setdiff1d(np.arange(len(head)), bad).tolist():
            state = c["ref_of"](tuple(x[i:i + 1] for x in r), *q, state=state, rule_base=i)
        return state

    # 1. rule ids: a step's relation past the table and below it, an empty and a reversed lag range, a head that is no relation
    body[1, 1], body[3, 0] = n_rela, -1
    lo[5, 2], hi[5, 2] = 8, 8
    lo[7, 0], hi[7, 0] = 15, 4
    head[-1] = 2 ** 31 - 1                                                       # sorted still: the largest head
    bad = [1, 3, 5, 7, len(head) - 1]
    ref = ref_without(bad)
    assert not XA.same(ref, full) and (ref[3] > 0).any()                         # the rules made bad did fire before
    assert XA.same(Raw(c, c["graph"], r, q).call(), ref)
    # 2. one query's row index is ``batch``, another's is -1: those rows stay at their initial values
    raw = Raw(c, c["graph"], r, q)
    lost = np.nonzero(ref[3].sum(1) > 0)[0][:2]
    raw.q_row = raw.q_row.copy()
    raw.q_row[np.isin(raw.q_row, lost)] = [B, -1]
    exp = tuple(a.copy() for a in ref)
    for a, init in zip(exp, A.initial(1, c["n_ent"])):
        a[lost] = init[0]
    assert XA.same(raw.call(), exp)
    # 3. a subject outside 0..n_ent-1 seeds nothing: its row fires nowhere
    raw = Raw(c, c["graph"], r, q)
    p = int(np.nonzero(raw.q_row == lost[0])[0][0])
    raw.q_sub = raw.q_sub.copy()
    raw.q_sub[p] = c["n_ent"]
    exp = tuple(a.copy() for a in ref)
    for a, init in zip(exp, A.initial(1, c["n_ent"])):
        a[lost[0]] = init[0]
    assert XA.same(raw.call(), exp)
    # 4. a row day out of range, on either side: the row is skipped.  The reference sees the same data with that row's relation set to
    # one that no rule names
    for j, d in ((3000, c["n_day"]), (3000, -1), (17, 2 ** 31 - 1)):
        raw = Raw(c, c["graph"], r, q)
        raw.row_day = c["row_day"].copy()
        raw.row_day[j] = d
        gone = c["data"].copy()
        gone[j, 1] = 99
        state = None
        for i in np.setdiff1d(np.arange(len(head)), bad).tolist():
            state = XA.apply_lists(c["n_ent"], c["n_rel"], gone, c["row_day"], c["lo"], c["hi"], *(x[i:i + 1] for x in r), *q, state=state,
                                   rule_base=i)
        assert XA.same(raw.call(), state), (j, d)
    # 5. the layout arrays of ONE relation made bad: day_of values outside 0..n_day-1, day_pos values outside 0..batch, day_ptr
    # entries outside 0..n_qdays, a slab outside 0..n_words.  The rules of the other heads are the reference's, cell for cell; the
    # call returns and the rows of the bad relation hold something
    victim = int(head[len(head) // 2])
    assert (q[1] == victim).any() and (q[1] == victim + 1).any() and (head == victim + 1).any()

    def spoil(name, values, affected=(victim,)):
        raw = Raw(c, c["graph"], r, q)
        k0, k1 = int(raw.day_ptr[victim]), int(raw.day_ptr[victim + 1])
        arr = getattr(raw, name).copy()
        if name == "day_of":
            arr[k0:k1] = np.resize(values, k1 - k0)
        elif name == "day_pos":
            arr[k0 + 1:k1] = np.resize(values, k1 - k0 - 1)                      # (the first belongs to the relation before as its end)
        elif name == "day_ptr":
            arr[victim + 1] = values
        elif name == "slab":
            arr[np.nonzero(head == victim)[0]] = values
        setattr(raw, name, arr)
        got = raw.call()
        others = ref_without(bad + np.nonzero(np.isin(head, affected))[0].tolist())
        rows_ok = np.nonzero(~np.isin(q[1], affected))[0]
        assert (others[3][rows_ok] > 0).any()
        assert XA.same(tuple(a[rows_ok] for a in got), tuple(a[rows_ok] for a in others)), (name, values)

    spoil("day_of", [c["n_day"], -1, 2 ** 31 - 1, -2 ** 31])
    spoil("day_of", [219, 1, 300, 0])                                            # unsorted, and past the last day
    spoil("day_pos", [-7, B + 1, 2 ** 31 - 1, 0])
    spoil("day_ptr", 2 ** 31 - 1, (victim, victim + 1))                          # the end of one relation's entries is the next one's start
    spoil("day_ptr", -1, (victim, victim + 1))
    spoil("slab", -1)
    spoil("slab", 2 ** 40)
    assert XA.same(Raw(c, c["graph"], r, q).call(), ref)                          # the process is as usable as before


# ---- the model entry points -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_case(case):
    """A table mined with rules(k = 3) from 60 rows of the fixture's data, its quality on the default anchors, and held-out queries:
    140 late rows (days 124..219) and two on days with empty windows."""
    c = case
    model, data = c["model"], c["data"]
    mine = data[np.arange(300, 6000, 95)]
    table = model.rules_all(mine, k=3, batch_size=32)
    quality = model.rule_quality(table)
    held = np.concatenate([data[np.arange(3400, 6000, 19)], data[c["row_day"] == 52][:1], data[c["row_day"] == 121][:1]], 0)
    assert len(held) >= 130 and table.head.numel() >= 20
    rules = (table.head.cpu().numpy(), table.body.cpu().numpy()) + X.bin_ranges(table.lag_bin.cpu().numpy())
    return dict(c, mine=mine, table=table, quality=quality, held=held, table_rules=rules, counts={})


def _ref_weights(m, rules, anchors=None, by_pca=False, laplace=0.0, min_hits=1):
    """(rows kept, their weights, the kept rules) of rule_scores restated from the reference counts."""
    key = tuple(x.tobytes() for x in rules) + (None if anchors is None else np.asarray(anchors).tobytes(),)
    if key not in m["counts"]:                                                   # the reference counts, once per (rules, anchors)
        m["counts"][key] = X.counts(*m["base"], *rules, anchors)
    cnt = m["counts"][key]
    den = cnt[:, 2 if by_pca else 0] + float(laplace)
    w = np.where(den > 0, cnt[:, 1] / np.where(den > 0, den, 1.0), 0.0).astype(np.float32)
    rows = np.nonzero((cnt[:, 1] >= min_hits) & (w > 0))[0]
    return rows, w[rows], tuple(x[rows] for x in rules)


def _ref_scores(m, rules, q, **kw):
    rows, w, kept = _ref_weights(m, rules, **kw)
    ref = XA.apply_lists(*m["base"], *kept, w, q[:, 0], q[:, 1], q[:, 3] // 24)
    rule = np.where(ref[2] >= 0, rows[np.maximum(ref[2], 0)], -1).astype(np.int32)
    return rows, (ref[0], ref[1], rule, ref[3])


def test_model_rule_scores_and_predict(model_case):
    from red_gnn_amd.explain import LagRuleTable, RulePrediction, RuleScores
    from red_gnn_amd.extrapolation import known_objects_index
    m = model_case
    model, table, quality, q = m["model"], m["table"], m["quality"], m["held"]
    X_b = ER.Batch(q)
    sp = known_objects_index(m["data"], model.n_rel, False)
    spt = known_objects_index(m["data"], model.n_rel, True)
    for kw, ref_kw in ((dict(), dict()), (dict(by="pca_confidence", laplace=2.0, min_hits=2), dict(by_pca=True, laplace=2.0, min_hits=2))):
        rows, ref = _ref_scores(m, m["table_rules"], q, **ref_kw)
        assert 0 < len(rows) <= table.head.numel()
        rs = model.rule_scores(quality, X_b, **kw)
        assert isinstance(rs, RuleScores) and np.array_equal(rs.rows.cpu().numpy(), rows)
        _check_types((rs.best, rs.surv, rs.best_rule, rs.fired), len(q), m["n_ent"])
        assert XA.same(_np((rs.best, rs.surv, rs.best_rule, rs.fired)), ref)       # best_rule holds table rows
        assert np.array_equal(rs.covered().cpu().numpy(), ref[3] > 0) and (ref[3] > 0).any() and (ref[3] >= 2).any()
        assert np.isin(ref[2][ref[2] >= 0], rows).all()
        small = model.rule_scores(quality, X_b, scratch_bytes=0, **kw)
        assert all(torch.equal(getattr(rs, f), getattr(small, f)) for f in ("best", "surv", "best_rule", "fired"))
        for agg, kn in (("noisy_or", spt), ("max", sp), ("noisy_or", None)):
            k = 7
            pred = model.rule_predict(quality, X_b, k=k, agg=agg, known=kn, **kw)
            assert isinstance(pred, RulePrediction) and pred.table is table and isinstance(pred.table, LagRuleTable)
            assert [t.dtype for t in (pred.ids, pred.scores, pred.rule, pred.fired)] == [torch.int64, torch.float32, torch.int64, torch.int32]
            assert all(t.shape == (len(q), k) and t.is_cuda for t in (pred.ids, pred.scores, pred.rule, pred.fired))
            sc = A.scores(ref[0], ref[1], agg)
            ids, val, rule, fired = (t.cpu().numpy() for t in (pred.ids, pred.scores, pred.rule, pred.fired))
            dropped = 0
            for b in range(len(q)):
                drop = [] if kn is None else kn.objects(q[b, 0], q[b, 1], q[b, 3])
                dropped += len(drop)
                top = A.order(sc[b], drop)[:k]
                assert np.array_equal(ids[b], top)
                assert np.array_equal(val[b].view(np.int32), sc[b, top].view(np.int32))
                assert np.array_equal(rule[b], ref[2][b, top]) and np.array_equal(fired[b], ref[3][b, top])
            assert dropped >= len(q) or kn is None                               # every held row is a fact: its own object is known
            assert len(pred.format()) == len(q) * k
    lines = model.rule_predict(quality, X_b, k=3).format(id2rel=["rel%d" % i for i in range(model.n_rel)])
    assert all(ln.startswith("row ") for ln in lines) and any("rel" in ln and "->" in ln and "d](" in ln for ln in lines)
    none = model.rule_predict(quality, ER.Batch(q[:0]), k=4)                     # a batch without rows
    assert all(t.shape == (0, 4) and t.is_cuda for t in (none.ids, none.scores, none.rule, none.fired))
    assert model.rule_scores(quality, ER.Batch(q[:0])).best.shape == (0, m["n_ent"])


def _filter_sets(q, index):
    lists = [sorted({int(o)} | (set() if index is None else set(index.objects(s, p, t).tolist()))) for s, p, o, t in q.tolist()]
    return np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32), np.concatenate(lists).astype(np.int32)


def _ref_metrics(m, rules, q, agg, sp, spt, **kw):
    rows, ref = _ref_scores(m, rules, q, **kw)
    sc = A.scores(ref[0], ref[1], agg)
    n = len(q)
    ap, ai = np.arange(n + 1, dtype=np.int32), q[:, 2].astype(np.int32)
    out = {"n": n, "coverage": float((ref[3][np.arange(n), q[:, 2]] > 0).sum()) / n}
    ranks = {}
    for sfx, index in (("", None), ("_fil_t", spt), ("_fil", sp)):
        fp, fi = _filter_sets(q, index)
        rank = ranks[sfx] = rank_ref.ranks(sc, ap, ai, fp, fi)
        out["hits1" + sfx], out["hits3" + sfx], out["hits10" + sfx] = (float(np.sum(rank <= c) / n) for c in (1, 3, 10))
        out["mrr" + sfx], out["mr" + sfx] = float(np.sum(1.0 / rank) / n), float(np.sum(rank) / n)
    return out, ranks


def test_rule_evaluate(model_case):
    from red_gnn_amd.extrapolation import known_objects_index
    m = model_case
    model, quality, q = m["model"], m["quality"], m["held"]
    sp = known_objects_index(m["data"], model.n_rel, False)
    spt = known_objects_index(m["data"], model.n_rel, True)
    for agg in ("noisy_or", "max"):
        ref, ranks = _ref_metrics(m, m["table_rules"], q, agg, sp, spt)
        assert 0 < ref["coverage"] <= 1 and (ranks["_fil"] <= ranks[""]).all() and (ranks["_fil_t"] <= ranks[""]).all()
        for batch_size in (256, 11):
            out = model.rule_evaluate(q, quality, agg=agg, sp_index=sp, spt_index=spt, batch_size=batch_size)
            assert set(out) == set(ref) and len(out) == 17
            assert out == ref, (agg, batch_size)
        raw = model.rule_evaluate(torch.as_tensor(q), quality, agg=agg)            # no index: the three ranks coincide
        assert all(raw[k] == raw[k + "_fil"] == raw[k + "_fil_t"] == ref[k] for k in ("hits1", "hits3", "hits10", "mrr", "mr"))
    # mine=: rules_all -> rule_quality on the default anchors BEFORE the earliest query day -> rule_evaluate(quality=...)
    late = q[q[:, 3] // 24 >= 124]
    first_day = int((late[:, 3] // 24).min())
    before = m["default"][m["default"][:, 1] < first_day]
    assert first_day >= 124 and 0 < len(before) < len(m["default"])
    table = model.rules_all(m["mine"], k=2)
    rules = (table.head.cpu().numpy(), table.body.cpu().numpy()) + X.bin_ranges(table.lag_bin.cpu().numpy())
    a = model.rule_evaluate(late, mine=m["mine"], k=2, sp_index=sp, spt_index=spt, laplace=1.0)
    by_hand = model.rule_quality(table, anchors=before)
    assert by_hand.n_anchors == len(before)
    assert a == model.rule_evaluate(late, quality=by_hand, sp_index=sp, spt_index=spt, laplace=1.0)
    want, _ = _ref_metrics(m, rules, late, "noisy_or", sp, spt, anchors=before, laplace=1.0)
    assert a == want and a["coverage"] > 0 and a["n"] == len(late)
    uncut, _ = _ref_metrics(m, rules, late, "noisy_or", sp, spt, laplace=1.0)
    assert not np.array_equal(_ref_weights(m, rules, before, laplace=1.0)[1], _ref_weights(m, rules, laplace=1.0)[1])      # the cut matters
    assert model.rule_evaluate(late, mine=m["mine"], k=2, sp_index=sp, spt_index=spt, laplace=1.0, anchors=m["default"]) == uncut
    # other lag edges reach the mining
    e = model.rule_evaluate(late, mine=m["mine"], k=2, lag_edges=(3, 30, 130))
    t3 = model.rules_all(m["mine"], k=2, lag_edges=(3, 30, 130))
    assert e == model.rule_evaluate(late, quality=model.rule_quality(t3, anchors=before))
    # a query on day 0: no anchor lies before it
    with pytest.raises(ValueError, match="rule_evaluate: no anchor lies before the earliest query day 0"):
        model.rule_evaluate(np.array([[0, 0, 1, 5]]), mine=m["mine"])


def test_model_errors(model_case):
    from red_gnn_amd.explain import LagRuleQuality, LagRuleTable, TemporalRuleQuality, TemporalRuleTable
    m = model_case
    model, quality, t, q = m["model"], m["quality"], m["table"], m["held"][:4]
    X_b = ER.Batch(q)
    counts = (quality.body_pairs, quality.hits, quality.pca_body_pairs, quality.head_pairs)
    temporal = TemporalRuleQuality(TemporalRuleTable(t.head, t.body, t.lag_bin.clamp(max=3), t.support, t.fixed, t.n_rel), *counts, 7)
    wrong = LagRuleQuality(LagRuleTable(t.head, t.body, t.lag_bin, t.support, t.fixed, t.lag_edges, t.n_rel + 1), *counts, 7)
    for name, call in (("rule_scores", lambda x: model.rule_scores(x, X_b)), ("rule_predict", lambda x: model.rule_predict(x, X_b)),
                       ("rule_evaluate", lambda x: model.rule_evaluate(q, x))):
        for bad in (temporal, t, None if name != "rule_evaluate" else 5):
            with pytest.raises(ValueError, match="%s: quality must be an explain.LagRuleQuality" % name):
                call(bad)
        with pytest.raises(ValueError, match="%s: the table has n_rel=%d, the model n_rel=%d" % (name, t.n_rel + 1, t.n_rel)):
            call(wrong)
    with pytest.raises(ValueError, match="rule_predict: agg must be"):
        model.rule_predict(quality, X_b, agg="mean")
    for k in (0, 1025, 2.0, True):
        with pytest.raises(ValueError, match="rule_predict: k must be an integer in 1"):
            model.rule_predict(quality, X_b, k=k)
    with pytest.raises(ValueError, match="rule_predict: known must be a KnownObjects index"):
        model.rule_predict(quality, X_b, known=(1, 2, 3))
    bad_t = ER.Batch(q.copy())
    bad_t.ts = q[:, 3] + 24 * m["n_day"]
    with pytest.raises(ValueError, match="rule_scores: query time outside the model's data"):
        model.rule_scores(quality, bad_t)
    with pytest.raises(ValueError, match="rule_scores: by must be"):
        model.rule_scores(quality, X_b, by="hits")
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
    with pytest.raises(ValueError, match="rule_evaluate: queries must be"):
        model.rule_evaluate(q[:, :3], quality)
    with pytest.raises(ValueError, match="rule_evaluate: sp_index must be a KnownObjects index"):
        model.rule_evaluate(q, quality, sp_index=(1, 2, 3))
