"""engine.xrule_ground (rg_xrule_ground, csrc/xrule_ground.hip) and extrapolation.T_RED_GNN.rules / rules_all / rule_quality on the
MI355X (-m gpu): every count equal, as an integer, to tests/xrule_ground_ref.py on the data the device graph was built from - the hand
data set with its typed-in counts, the 150-entity fixture under random rules of every bin with the default anchors (more words than a
wave), entity x day anchors on the days with empty windows and with windows from row 0, subsets around the word boundaries, the
smallest chunking, other path lengths, the model's own rules, the errors, and the kernel's own bounds on its ids."""
import numpy as np
import pytest
import torch

from tests import extrap_ref as ER
from tests import xrule_ground_ref as X

pytestmark = pytest.mark.gpu

SUBSET_SIZES = (1, 31, 32, 33, 64, 65)


def _invariants(c):
    assert (c >= 0).all()
    assert (c[:, 1] <= c[:, 2]).all() and (c[:, 2] <= c[:, 0]).all() and (c[:, 1] <= c[:, 3]).all()


def test_hand_data_set():
    from red_gnn_amd import engine
    n_data = len(X.HAND_DATA)
    g = engine.TemporalGraph(X.HAND_N_ENT, X.HAND_N_REL + 1, n_data + 1, X.graph_rows(X.HAND_DATA, X.HAND_N_ENT, X.HAND_N_REL))
    assert g.n_fact == n_data + X.HAND_N_ENT
    lo, hi = X.windows(X.HAND_OFF)
    rules = X.hand_rules()
    ground = lambda r, a=None, **kw: engine.xrule_ground(g, r[0], r[1], r[2], r[3], X.HAND_ROW_DAY, lo, hi, a, **kw)
    got = ground(rules)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (7, 4)
    got = got.cpu().numpy()
    assert np.array_equal(got, X.HAND_ALL)
    assert np.array_equal(got, X.counts_dense(X.HAND_N_ENT, X.HAND_N_REL, X.HAND_DATA, X.HAND_ROW_DAY, lo, hi, *rules))
    assert np.array_equal(ground(rules, X.HAND_ANCHORS).cpu().numpy(), X.HAND_ALL)      # the default anchors, spelled out
    assert got[3].tolist() == [0, 0, 0, got[0, 3]] and got[0, 3] > 0                      # a step over a relation without rows
    dev = lambda x: torch.as_tensor(x).cuda()
    sub = engine.xrule_ground(g, dev(rules[0]), dev(rules[1]), dev(rules[2]), dev(rules[3]), dev(X.HAND_ROW_DAY), dev(lo), dev(hi),
                              torch.as_tensor(X.HAND_SUBSET, dtype=torch.int32))
    assert np.array_equal(sub.cpu().numpy(), X.HAND_SUB)
    # a self-loop's lag is min(t, loop_window): with loop_window = 4 the self-loops of days 4, 122 and 123 land in the bin 4-7d
    loop = (np.array([1]), np.array([[3]]), np.array([[4]]), np.array([[8]]))
    for lw in (120, 4, 0):
        want = X.counts(X.HAND_N_ENT, X.HAND_N_REL, X.HAND_DATA, X.HAND_ROW_DAY, lo, hi, *loop, None, lw)
        assert np.array_equal(ground(loop, loop_window=lw).cpu().numpy(), want), lw
        assert want[0, 0] == {120: 2, 4: 6, 0: 0}[lw]
    empty = ground(tuple(x[:0] for x in rules))
    assert empty.is_cuda and empty.shape == (0, 4) and empty.dtype == torch.int64
    assert not ground(rules, np.zeros((0, 2), np.int64)).any()


@pytest.fixture(scope="module")
def case():
    """extrap_ref.make_case(32, 9): 150 entities, 6 relations + the identity (the graph has the 8 rows of the model's relation table),
    6000 rows over 220 days; the graph, row days and offsets are the model's own (make_model).  40 random rules (L = 1, 2, 3; every bin, ANY and identity steps) and the anchor sets of the tests."""
    from red_gnn_amd import engine
    data, queries = ER.make_case(32, 9)
    model = ER.make_model(data, 32, 5, "tanh", 3)
    n_ent, n_rel = ER.N_ENT, ER.N_REL
    assert model.n_rel_true == n_rel and model.graph.n_rela_rows == n_rel + 2 and model.graph.n_time == len(data) + 1
    row_day, off = model.row_time.cpu().numpy().astype(np.int64), model.time_offset_list
    assert np.array_equal(row_day, data[:, 3] // 24) and np.array_equal(off, X.offsets(row_day))
    assert np.nonzero(off == 0)[0].tolist() == [0, 1, 51, 52, 121]
    lo, hi = X.windows(off)
    n_day = len(off)
    rules = X.random_rules(np.random.default_rng(17), 40, n_rel + 1)
    default = X.default_anchors(data, row_day, n_ent)
    assert len(default) == 4062 and (len(default) + 31) // 32 == 127 and len(default) % 32 != 0
    days = np.unique(np.concatenate([np.arange(0, n_day, 5), [1, 52, 121, 171, 172]]))
    every = np.stack(np.meshgrid(np.arange(n_ent), days, indexing="ij"), -1).reshape(-1, 2)
    ref = lambda r, a=None: X.counts(n_ent, n_rel, data, row_day, lo, hi, r[0], r[1], r[2], r[3], a)

    def ground(r, a=None, **kw):
        got = engine.xrule_ground(model.graph, r[0], r[1], r[2], r[3], row_day, lo, hi, a, **kw)
        assert got.is_cuda and got.dtype == torch.int64 and got.shape == (len(r[0]), 4)
        return got.cpu().numpy()
    return dict(model=model, graph=model.graph, data=data, queries=queries, n_ent=n_ent, n_rel=n_rel, n_day=n_day, row_day=row_day, lo=lo,
                hi=hi, rules=rules, default=default, every=every, ref=ref, ground=ground, ref_default={L: ref(r) for L, r in rules.items()})


def test_default_anchors_random_rules(case):
    c = case
    assert np.array_equal(c["model"].default_anchors(), c["default"])
    got = []
    for L, r in c["rules"].items():
        g = c["ground"](r)
        assert np.array_equal(g, c["ref_default"][L]), L
        _invariants(g)
        got.append(g)
        if L == 2:                             # the definition itself on a part of the anchors (the dense form is slow beyond a few hundred)
            part = np.concatenate([c["default"][100:250], c["default"][-120:]], 0)
            assert np.array_equal(c["ground"](r, part), X.counts_dense(c["n_ent"], c["n_rel"], c["data"], c["row_day"], c["lo"], c["hi"],
                                                                      *r, part))
    got = np.concatenate(got, 0)
    body = np.concatenate([r[1].reshape(-1) for r in c["rules"].values()])
    lag_lo = np.concatenate([r[2].reshape(-1) for r in c["rules"].values()])
    lag_hi = np.concatenate([r[3].reshape(-1) for r in c["rules"].values()])
    assert len(got) == 40 and (body == c["n_rel"]).any()
    assert set(lag_lo.tolist()) == {0, 2, 4, 8, 15, 31, 61, 121} and ((lag_lo == 0) & (lag_hi == X.ANY_HI)).any()      # every bin, and ANY
    assert (got[:, 0] > 0).sum() >= 20 and (got[:, 1] > 0).sum() >= 10           # not a comparison of zeros
    assert ((got[:, 1] > 0) & (got[:, 1] < got[:, 0])).any()
    old, at = [], 0
    for L, r in c["rules"].items():            # a rule with a data-row step in the 121+ bin that grounds
        old += [at + i for i in range(len(r[0])) if ((r[2][i] == 121) & (r[1][i] != c["n_rel"])).any()]
        at += len(r[0])
    assert old and (got[old, 0] > 0).any()


def test_entity_day_anchors_on_empty_windows_and_windows_from_row_0(case):
    c = case
    assert (len(c["every"]) + 31) // 32 > 64
    for L, r in c["rules"].items():
        got = c["ground"](r, c["every"])
        assert np.array_equal(got, c["ref"](r, c["every"])), L
        _invariants(got)
    on = lambda t: np.column_stack([np.arange(c["n_ent"]), np.full(c["n_ent"], t)])
    any_lo, any_hi = np.zeros((1, 2), np.int64), np.full((1, 2), X.ANY_HI)
    rows_only = (np.array([0]), np.array([[1, 2]]), any_lo, any_hi)
    loops_only = (np.array([0]), np.array([[c["n_rel"]] * 2]), any_lo, any_hi)
    for t in (1, 52, 121):                     # off[t] == 0: the window is empty, only the self-loops are there
        assert c["lo"][t] >= c["hi"][t]
        assert c["ground"](rows_only, on(t))[0, 0] == 0 and c["ground"](loops_only, on(t))[0, 0] == c["n_ent"]
    for t in (171, 172):                       # off[t - 120] == 0: the window starts at row 0
        assert c["lo"][t] == 0 and c["hi"][t] > 0 and t - c["row_day"][0] > 120
    old = (np.array([0, 1]), np.array([[2], [3]]), np.full((2, 1), 121), np.full((2, 1), X.ANY_HI))
    got = c["ground"](old, on(171))
    assert np.array_equal(got, c["ref"](old, on(171))) and (got[:, 0] > 0).all()
    # a full window starts at the last row of the day before its first day: one row of lag 121, and no older one
    assert c["lo"][170] > 0 and 170 - c["row_day"][c["lo"][170]] == 121
    assert np.array_equal(c["ground"](old, on(170)), c["ref"](old, on(170)))


@pytest.mark.parametrize("n", SUBSET_SIZES)
def test_anchor_subsets_around_the_word_boundaries(case, n):
    c = case
    rng = np.random.default_rng(100 + n)
    anchors = c["every"][rng.permutation(len(c["every"]))[:n]]
    r = c["rules"][2]
    got = c["ground"](r, anchors)
    assert np.array_equal(got, c["ref"](r, anchors))
    _invariants(got)


def test_day_ranges_on_word_boundaries(case):
    c = case
    rng = np.random.default_rng(7)
    at = lambda t, k: np.column_stack([rng.permutation(c["n_ent"])[:k], np.full(k, t)])
    sets = dict(three_full_words=np.concatenate([at(60, 32), at(61, 32), at(172, 32)], 0),      # every day's columns start and end on a boundary
                one_full_word=at(100, 32), two_full_words=at(171, 64))
    for name, anchors in sets.items():
        some = 0
        for L, r in c["rules"].items():
            got = c["ground"](r, anchors)
            assert np.array_equal(got, c["ref"](r, anchors)), (name, L)
            some += int(got[:, 0].sum())
        assert some > 0, name


def test_chunking_changes_no_count(case):
    from red_gnn_amd import engine
    c = case
    small = engine.rule_ground_scratch_bytes(c["n_ent"], 1, 32)
    assert engine.rule_chunking(c["n_ent"], 14, len(c["default"]), small) == (1, 32)
    for L, r in c["rules"].items():
        assert np.array_equal(c["ground"](r, scratch_bytes=small), c["ref_default"][L]), L
    r = c["rules"][3]
    mid = engine.rule_ground_scratch_bytes(c["n_ent"], 5, 96)                   # 5 rules x 96 anchors
    assert np.array_equal(c["ground"](r, scratch_bytes=mid), c["ref_default"][3])
    events = engine.XRULE_EVENTS = []
    try:
        c["ground"](r, scratch_bytes=small)
    finally:
        engine.XRULE_EVENTS = None
    assert len(events) == len(r[0]) * 127 and {e[3] for e in events} == {32, 4062 - 126 * 32} and {e[2] for e in events} == {1}


@pytest.mark.parametrize("L", [1, 4])
def test_other_path_lengths(case, L):
    c = case
    rng = np.random.default_rng(200 + L)
    bins = np.where(rng.integers(0, 2, (20, L)) == 0, 8, rng.integers(0, 8, (20, L)))
    r = (rng.integers(0, c["n_rel"], 20), rng.integers(0, c["n_rel"] + 1, (20, L))) + X.bin_ranges(bins)
    for anchors in (None, c["every"][::7]):
        got = c["ground"](r, anchors)
        assert np.array_equal(got, c["ref"](r, anchors))
        _invariants(got)
        assert (got[:, 0] > 0).any()


def _same_table(a, b):
    a, b = a.cpu(), b.cpu()
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "lag_bin", "support", "fixed")) \
        and a.n_rel == b.n_rel and a.lag_edges == b.lag_edges


def _counts_of(q):
    return torch.stack([q.body_pairs, q.hits, q.pca_body_pairs, q.head_pairs], 1).cpu().numpy()


def test_model_rules_and_quality(case):
    """The kernel's window and lag convention is the forward's: a path the model explains for (subject, day) -> answer grounds its own
    rule at that anchor, so each rule's body_pairs is at least the number of distinct (anchor, answer) rows that gave it."""
    from red_gnn_amd import profile
    from red_gnn_amd.explain import LagRuleQuality, LagRuleTable
    c = case
    model, data, k = c["model"], c["data"], 3
    q = np.concatenate([c["queries"], data[[150, 2000, 3500, 4400, 5990]]], 0)
    batch = ER.Batch(q)
    day = q[:, 3] // 24
    objs = model.predict(batch, k=1).ids[:, 0].cpu().numpy()
    assert (objs >= 0).all()
    table = model.rules(batch, objs, k=k)
    assert isinstance(table, LagRuleTable) and table.n_rel == model.n_rel_true == model.n_rel - 1 and table.body.shape[1] == 3
    assert table.lag_edges == profile.DEFAULT_LAG_EDGES and table.head.numel() > 3
    assert _same_table(table, model.rules(batch, k=k))                            # objs defaults to each row's own top forecast
    # the rows behind every rule, from the same paths
    ps = model.explain(batch, objs).top_paths(k)
    rel = ps.rels().cpu().numpy()
    lag = ps._gather(ps.digraph.lag().long(), 0).cpu().numpy()
    b = profile.lag_bins(lag, table.lag_edges)
    b[rel == model.n_rel_true] = table.any_bin
    count = ps.count.cpu().numpy()
    assert int(table.support.sum()) == int(count.sum()) and count.sum() >= len(q)
    assert ((ps.data_rows().cpu().numpy() < 0) == ((rel == model.n_rel_true) | (rel < 0))).all()
    behind = {}
    for i in range(len(q)):
        for j in range(count[i]):
            key = (int(q[i, 1]),) + tuple(np.stack([rel[i, j], b[i, j]], 1).reshape(-1).tolist())
            behind.setdefault(key, set()).add((int(q[i, 0]), int(day[i]), int(objs[i])))
    keys = [tuple(x) for x in table.key().cpu().tolist()]
    assert sorted(behind) == keys
    assert len(set(b[(rel != model.n_rel_true) & (rel >= 0)].tolist())) >= 3     # steps of several lag bins occur
    anchors = np.unique(np.column_stack([q[:, 0], day]), axis=0)
    qual = model.rule_quality(table, anchors=anchors)
    assert isinstance(qual, LagRuleQuality) and qual.table is table and qual.n_anchors == len(anchors) and qual.hits.is_cuda
    got = _counts_of(qual)
    low = np.array([len(behind[key]) for key in keys])
    assert (low > 0).all() and (got[:, 0] >= low).all()
    rules = (table.head.cpu().numpy(), table.body.cpu().numpy()) + tuple(x.cpu().numpy() for x in table.lag_ranges())
    assert np.array_equal(rules[2:], X.bin_ranges(table.lag_bin.cpu().numpy()))
    assert np.array_equal(got, c["ref"](rules, anchors))
    _invariants(got)
    assert not qual.trivial().any() and len(qual.format()) == len(keys) and (qual.confidence() <= 1.0).all()
    # the default anchors, and a budget that forces chunks
    full = model.rule_quality(table, scratch_bytes=1 << 16)
    assert full.n_anchors == len(c["default"])
    assert np.array_equal(_counts_of(full), c["ref"](rules))
    # other lag edges: other bins, the same reference
    other = model.rules(batch, objs, k=k, lag_edges=(3, 30, 130))
    assert other.lag_edges == (3, 30, 130) and int(other.support.sum()) == int(count.sum())
    o_rules = (other.head.cpu().numpy(), other.body.cpu().numpy()) + X.bin_ranges(other.lag_bin.cpu().numpy(), (3, 30, 130))
    assert np.array_equal([x.cpu().numpy() for x in other.lag_ranges()], o_rules[2:])
    assert np.array_equal(_counts_of(model.rule_quality(other, anchors=anchors)), c["ref"](o_rules, anchors))
    # rules_all: the sum of the per-batch tables, the objects being the answers
    parts = None
    for lo in range(0, len(q), 4):
        part = q[lo:lo + 4]
        t = model.rules(ER.Batch(part), part[:, 2], k=2)
        parts = t if parts is None else parts + t
    assert _same_table(model.rules_all(q, k=2, batch_size=4), parts) and parts.head.numel() > 0
    assert _same_table(model.rules_all(torch.as_tensor(q), k=2, batch_size=64), parts)
    with pytest.raises(ValueError, match="rule_quality: table must be an explain.LagRuleTable"):
        model.rule_quality(None)
    with pytest.raises(ValueError, match="rule_quality: the table has n_rel=%d, the model n_rel=%d" % (model.n_rel, model.n_rel_true)):
        model.rule_quality(LagRuleTable(table.head, table.body, table.lag_bin, table.support, table.fixed, table.lag_edges, model.n_rel))
    with pytest.raises(ValueError, match="rules_all: queries must be"):
        model.rules_all(q[:, :3])
    with pytest.raises(ValueError, match="lag_edges"):
        model.rules(batch, objs, lag_edges=(4, 4))
    with pytest.raises(ValueError, match="xrule_ground: anchor out of range"):
        model.rule_quality(table, anchors=np.array([[0, c["n_day"]]]))


def _raw(c, graph, head, body, lag_lo, lag_hi, anchors, row_day=None, n_rules=None, n_hops=None, n_anchors=None, n_data=None):
    """rg_xrule_ground itself on sorted anchors int64 [S, 2]: the counts int64 [R, 4] as numpy."""
    from red_gnn_amd import _lib, engine
    dev = torch.device("cuda")
    t32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    S, R, L = len(anchors), len(head), np.asarray(body).shape[1]
    row_day = c["row_day"] if row_day is None else row_day
    ptr = np.searchsorted(anchors[:, 1], np.arange(c["n_day"] + 1))
    h, b, lo, hi, day, wl, wh, e, pt = (t32(x) for x in (head, body, lag_lo, lag_hi, row_day, c["lo"], c["hi"], anchors[:, 0], ptr))
    counts = torch.zeros((R, 4), dtype=torch.int64, device=dev)
    scratch = torch.empty(max(engine.rule_ground_scratch_bytes(graph.n_ent, R, S), 4), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().rg_xrule_ground(graph.handle, p(h), p(b), p(lo), p(hi), R if n_rules is None else n_rules,
                                          L if n_hops is None else n_hops, p(day), len(row_day) if n_data is None else n_data, p(wl), p(wh),
                                          c["n_day"], 120, p(e), p(pt), S if n_anchors is None else n_anchors, p(scratch), p(counts),
                                          _lib.stream_ptr()))
    return counts.cpu().numpy()


def test_errors(case):
    from red_gnn_amd import _lib, engine
    c = case
    xg, r = c["graph"], tuple(x[:1] for x in c["rules"][2])
    one = c["default"][:1]
    sg = engine.Graph(5, 2, np.array([[0, 0, 1], [1, 1, 2], [3, 0, 4]]))
    with pytest.raises(_lib.NativeError, match="rg_xrule_ground: not the extrapolation layout"):
        _raw(c, sg, *r, one)
    tg = engine.TemporalGraph(5, 3, 4, np.array([[0, 0, 1, 0], [1, 1, 2, 3], [3, 2, 3, 3]]))      # an interpolation graph: 4 time ids
    with pytest.raises(_lib.NativeError, match=r"rg_xrule_ground: not the extrapolation layout \(n_time=4, n_data=6000"):
        _raw(c, tg, *r, one)
    for hops in (0, 33):
        with pytest.raises(_lib.NativeError, match="rg_xrule_ground: n_hops=%d not in 1..32" % hops):
            _raw(c, xg, *r, one, n_hops=hops)
    with pytest.raises(_lib.NativeError, match="rg_xrule_ground: n_rules=65536 not in"):
        _raw(c, xg, *r, one, n_rules=65536)
    with pytest.raises(_lib.NativeError, match="rg_xrule_ground: n_anchors=-1"):
        _raw(c, xg, *r, one, n_anchors=-1)
    assert not _raw(c, xg, *r, one, n_rules=0).any() and not _raw(c, xg, *r, one, n_anchors=0).any()
    assert np.array_equal(_raw(c, xg, *r, one), c["ref"](r, one))
    full = c["rules"][2]
    with pytest.raises(ValueError, match=r"xrule_ground: relation id out of range 0\.\.%d" % (xg.n_rela_rows - 1)):
        bad = full[1].copy()
        bad[0, 1] = xg.n_rela_rows
        c["ground"]((full[0], bad, full[2], full[3]))
    with pytest.raises(ValueError, match="xrule_ground: lag range out of order"):
        c["ground"]((full[0], full[1], full[3], full[2]))
    with pytest.raises(ValueError, match="xrule_ground: duplicate anchors"):
        c["ground"](full, np.array([[4, 1], [9, 0], [4, 1]]))
    with pytest.raises(ValueError, match="xrule_ground: not the extrapolation layout"):
        engine.xrule_ground(tg, *full, c["row_day"], c["lo"], c["hi"], one)


def test_ids_are_bounded_in_the_kernel(case):
    """The C entry point trusts its caller for the ids (engine.xrule_ground validates them): a rule whose step names a relation the
    graph does not have, or an empty lag range, grounds nothing; a data row whose day lies outside 0..n_day-1 is skipped as a step and
    as a head; the other rules of the call are counted as ever, and the process stays usable."""
    c = case
    head, body, lo, hi = (x.copy() for x in c["rules"][3])
    ref = c["ref_default"][3]
    n_rela = c["graph"].n_rela_rows                                                # 8: the model's table has one row past the identity
    assert len(head) >= 8 and (ref[:, 0] > 0).sum() >= 4
    body[1, 1], body[3, 0] = n_rela, -1
    lo[5, 2], hi[5, 2] = 8, 8                                                      # lag_lo >= lag_hi: an empty step
    lo[7, 0], hi[7, 0] = 15, 4
    head[6] = n_rela                                                               # no such head relation: the body is counted, no head
    got = _raw(c, c["graph"], head, body, lo, hi, c["default"])
    for i in (1, 3, 5, 7):
        assert got[i, :3].tolist() == [0, 0, 0] and got[i, 3] == ref[i, 3]
    assert got[6].tolist() == [ref[6, 0], 0, 0, 0]
    rest = [i for i in range(len(head)) if i not in (1, 3, 5, 6, 7)]
    assert np.array_equal(got[rest], ref[rest])
    # one row's day out of range, on either side: the row is skipped.  The reference sees the same data with that row's relation set
    # to one that no rule names.  The default anchors of the intact data are kept, so the row's own (subject, day) is still an anchor
    r = c["rules"][2]
    for j, bad in ((3000, c["n_day"]), (3000, -1), (17, 2 ** 31 - 1)):
        day = c["row_day"].copy()
        day[j] = bad
        gone = c["data"].copy()
        gone[j, 1] = 99
        want = X.counts(c["n_ent"], c["n_rel"], gone, c["row_day"], c["lo"], c["hi"], *r, c["default"])
        assert np.array_equal(_raw(c, c["graph"], *r, c["default"], row_day=day), want), (j, bad)
        assert not np.array_equal(want, c["ref_default"][2])                        # the row mattered
    assert np.array_equal(c["ground"](r), c["ref_default"][2])                      # the process is as usable as before
