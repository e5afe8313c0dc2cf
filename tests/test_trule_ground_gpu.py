"""engine.trule_ground (rg_trule_ground, csrc/trule_ground.hip) and T_RED_GNN.rules / rules_all / rule_quality on the MI355X (-m gpu):
every count equal, as an integer, to tests/trule_ground_ref.py on the quadruples the device graph was built from - the hand graph with
its typed-in counts, a 200-entity graph under random rules of every direction with the default anchors, all (entity, time) pairs (more
words than a wave), subsets around the word boundaries, anchor sets whose time ranges start and end on word boundaries or lie at one end
of the time axis, the smallest chunking, other path lengths, the model's own rules on its hand graph, the errors, and the kernel's own
bounds on relation ids and directions."""
import numpy as np
import pytest
import torch

from tests import layer_ref as LR
from tests import temporal_ref as TR
from tests import trule_ground_ref as T

pytestmark = pytest.mark.gpu

SUBSET_SIZES = (1, 31, 32, 33, 64, 65)


def _invariants(c):
    assert (c >= 0).all()
    assert (c[:, 1] <= c[:, 2]).all() and (c[:, 2] <= c[:, 0]).all() and (c[:, 1] <= c[:, 3]).all()


def _ground(graph, rules, anchors=None, **kw):
    from red_gnn_amd import engine
    got = engine.trule_ground(graph, rules[0], rules[1], rules[2], anchors, **kw)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (len(rules[0]), 4)
    return got.cpu().numpy()


def test_hand_graph():
    from red_gnn_amd import engine
    quads = T.hand_quads()
    g = engine.TemporalGraph(T.HAND_N_ENT, T.HAND_N_RELA, T.HAND_N_TIME, quads)
    assert g.n_fact == len(quads) and np.array_equal(g.default_anchors(), T.HAND_ANCHORS)
    rules = (T.HAND_HEAD, T.HAND_BODY, T.HAND_DIR)
    got = _ground(g, rules)
    assert np.array_equal(got, T.HAND_ALL)
    assert np.array_equal(got, T.counts_dense(T.HAND_N_ENT, T.HAND_N_RELA, T.HAND_N_TIME, quads, *rules))
    assert got[4].tolist() == [0, 0, 0, got[1, 3]] and got[1, 3] > 0            # a step over a relation without edges
    dev = lambda x: torch.as_tensor(x).cuda()
    sub = engine.trule_ground(g, dev(T.HAND_HEAD), dev(T.HAND_BODY), dev(T.HAND_DIR), torch.as_tensor(T.HAND_SUBSET, dtype=torch.int32))
    assert np.array_equal(sub.cpu().numpy(), T.HAND_SUB)
    empty = engine.trule_ground(g, T.HAND_HEAD[:0], T.HAND_BODY[:0], T.HAND_DIR[:0])
    assert empty.is_cuda and empty.shape == (0, 4) and empty.dtype == torch.int64
    assert not engine.trule_ground(g, *rules, np.zeros((0, 2), np.int64)).any()


@pytest.fixture(scope="module")
def case():
    """layer_ref._temporal_case(seed=2, B=9, m=600): 200 entities, 11 relation ids, 12 time ids, facts repeated at other times; its
    device graph, 40 random rules (L = 1, 2, 3; every direction; identity and inverse steps) and the anchor sets of the tests."""
    from red_gnn_amd import engine
    c = LR._temporal_case("trule", seed=2, B=9, m=600)
    n_ent, n_rela, n_time, quads = c.n_ent, c.n_rela_rows, c.n_time, c.quads
    assert (n_ent, n_rela, n_time) == (200, 11, 12)
    graph = engine.TemporalGraph(n_ent, n_rela, n_time, quads)
    rng = np.random.default_rng(17)
    rules = T.random_rules(rng, 40, n_rela)
    default = T.default_anchors(quads, n_ent, n_rela)
    assert len(default) == 895 and (len(default) + 31) // 32 == 28 and len(default) % 32 != 0
    every = np.stack(np.meshgrid(np.arange(n_ent), np.arange(n_time), indexing="ij"), -1).reshape(-1, 2)
    ref = lambda r, a=None: T.counts(n_ent, n_rela, n_time, quads, r[0], r[1], r[2], a)
    return dict(graph=graph, n_ent=n_ent, n_rela=n_rela, n_time=n_time, quads=quads, rules=rules, default=default, every=every, ref=ref,
                rng=rng, ref_default={L: ref(r) for L, r in rules.items()})


def test_default_anchors_random_rules(case):
    c = case
    assert np.array_equal(c["graph"].default_anchors(), c["default"])
    got = []
    for L, r in c["rules"].items():
        g = _ground(c["graph"], r)
        assert np.array_equal(g, c["ref_default"][L]), L
        _invariants(g)
        got.append(g)
        if L == 2:                             # the definition itself on a part of the anchors (the dense form is slow beyond a few hundred)
            part = c["default"][100:333]
            assert np.array_equal(_ground(c["graph"], r, part), T.counts_dense(c["n_ent"], c["n_rela"], c["n_time"], c["quads"], *r, part))
    got = np.concatenate(got, 0)
    direc = np.concatenate([r[2].reshape(-1) for r in c["rules"].values()])
    body = np.concatenate([r[1].reshape(-1) for r in c["rules"].values()])
    assert len(got) == 40 and set(direc.tolist()) == {0, 1, 2, 3} and (body == c["n_rela"] - 1).any()
    assert (got[:, 0] > 0).sum() >= 20 and (got[:, 1] > 0).sum() >= 10           # not a comparison of zeros
    assert ((got[:, 1] > 0) & (got[:, 1] < got[:, 0])).any()


def test_all_entity_time_pairs_more_words_than_a_wave(case):
    c = case
    assert (len(c["every"]) + 31) // 32 == 75
    for L, r in c["rules"].items():
        got = _ground(c["graph"], r, c["every"])
        assert np.array_equal(got, c["ref"](r, c["every"])), L
        _invariants(got)
        assert (got[:, 0] >= c["ref_default"][L][:, 0]).all()                   # the default anchors are among them


@pytest.mark.parametrize("n", SUBSET_SIZES)
def test_anchor_subsets_around_the_word_boundaries(case, n):
    c = case
    rng = np.random.default_rng(100 + n)
    anchors = c["every"][rng.permutation(len(c["every"]))[:n]]
    r = c["rules"][2]
    got = _ground(c["graph"], r, anchors)
    assert np.array_equal(got, c["ref"](r, anchors))
    _invariants(got)


def test_time_ranges_on_word_boundaries_and_at_the_ends(case):
    c = case
    rng = np.random.default_rng(7)
    ents = lambda k: rng.permutation(c["n_ent"])[:k]
    at = lambda t, k: np.column_stack([ents(k), np.full(k, t)])
    last = c["n_time"] - 1
    sets = dict(three_full_words=np.concatenate([at(0, 32), at(5, 32), at(last, 32)], 0),      # every range starts and ends on a boundary
                one_full_word=at(4, 32), two_full_words=at(6, 64),
                all_at_time_0=at(0, 70),                                                        # future: empty; past: every column
                all_at_last_time=at(last, 70))                                                  # past: empty; future: every column
    for name, anchors in sets.items():
        some = 0
        for L, r in c["rules"].items():
            got = _ground(c["graph"], r, anchors)
            assert np.array_equal(got, c["ref"](r, anchors)), (name, L)
            some += int(got[:, 0].sum())
        assert some > 0, name
    # the ends, stated outright: no edge lies in the past of an anchor at time 0, none in the future of one at the last time id
    head, rel = np.zeros(1, np.int64), np.zeros((1, 1), np.int64)
    for t, empty_dir, full_dir in ((0, T.PAST, T.FUTURE), (last, T.FUTURE, T.PAST)):
        anchors = at(t, 70)
        assert _ground(c["graph"], (head, rel, np.full((1, 1), empty_dir)), anchors)[0, 0] == 0
        now = _ground(c["graph"], (head, rel, np.full((1, 1), T.NOW)), anchors)[0, 0]
        other = _ground(c["graph"], (head, rel, np.full((1, 1), full_dir)), anchors)[0, 0]
        both = _ground(c["graph"], (head, rel, np.full((1, 1), T.ANY)), anchors)[0, 0]
        assert other > 0 and max(now, other) <= both <= now + other


def test_chunking_changes_no_count(case):
    from red_gnn_amd import engine
    c = case
    small = engine.trule_ground_scratch_bytes(c["n_ent"], 1, 32)
    assert engine.rule_chunking(c["n_ent"], 14, len(c["default"]), small) == (1, 32)
    for L, r in c["rules"].items():
        assert np.array_equal(_ground(c["graph"], r, scratch_bytes=small), c["ref_default"][L]), L
    r = c["rules"][3]
    mid = engine.trule_ground_scratch_bytes(c["n_ent"], 5, 96)                  # 5 rules x 96 anchors
    assert np.array_equal(_ground(c["graph"], r, scratch_bytes=mid), c["ref_default"][3])
    assert np.array_equal(_ground(c["graph"], r, c["every"], scratch_bytes=small), c["ref"](r, c["every"]))
    events = engine.TRULE_EVENTS = []
    try:
        _ground(c["graph"], r, scratch_bytes=small)
    finally:
        engine.TRULE_EVENTS = None
    assert len(events) == len(r[0]) * 28 and {e[3] for e in events} == {32, 895 - 27 * 32} and {e[2] for e in events} == {1}


@pytest.mark.parametrize("L", [1, 4])
def test_other_path_lengths(case, L):
    c = case
    rng = np.random.default_rng(200 + L)
    r = (rng.integers(0, c["n_rela"] - 1, 20), rng.integers(0, c["n_rela"], (20, L)), rng.integers(0, 4, (20, L)))
    for anchors in (None, c["every"][::7]):
        got = _ground(c["graph"], r, anchors)
        assert np.array_equal(got, c["ref"](r, anchors))
        _invariants(got)
        assert (got[:, 0] > 0).any()


def _same_table(a, b):
    a, b = a.cpu(), b.cpu()
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "direction", "support", "fixed")) and a.n_rel == b.n_rel


def test_model_rules_and_quality():
    """The kernel's direction convention is the forward's: a path the model explains for (head, time) -> answer grounds its own rule
    at that anchor, so each rule's body_pairs is at least the number of distinct (anchor, answer) rows that gave it."""
    from red_gnn_amd.explain import TemporalRuleQuality, TemporalRuleTable
    quads = TR.hand_graph()
    n_ent, n_rela, n_time, k = TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1, TR.HAND_N_TIME, 3
    model = TR.make_model(quads, n_ent, n_rela, n_time, 3, 16, 3, "relu")
    assert model.n_rel == n_rela - 1
    heads, rels, times = np.array([0, 1, 2, 3, 3, 260, 130]), np.array([0, 1, 2, 0, 4, 1, 5]), np.array([0, n_time - 1, 5, 5, 2, 4, 7])
    with torch.no_grad():
        model({"head": heads, "relation": rels, "time": times}, mode="test")
    nodes = model.last_nodes.cpu().numpy()
    q_of, objs = [], []
    for b in range(len(heads)):                      # two answers per query from its last level: the first and the last entity
        mine = nodes[nodes[:, 0] == b, 1]
        q_of += [b, b]
        objs += [int(mine[0]), int(mine[-1])]
    q_of, objs = np.array(q_of + [5]), np.array(objs + [70])      # every path 260 -> 70 takes the edge (260, 1, 70) of the query's own time 4
    batch = {"head": heads[q_of], "relation": rels[q_of], "time": times[q_of]}
    table = model.rules(batch, objs, k=k)
    assert isinstance(table, TemporalRuleTable) and table.n_rel == model.n_rel and table.body.shape[1] == 3 and table.head.numel() > 3
    assert _same_table(table, model.rules(dict(batch, tail=objs), k=k))         # objs defaults to the batch's tails
    # the rows behind every rule, from the same paths
    ps = model.explain(batch, objs).top_paths(k)
    rel = ps.rels().cpu().numpy()
    d = ps._gather(ps.digraph.direction().long(), -1).cpu().numpy()
    d[rel == model.n_rel] = 3
    count = ps.count.cpu().numpy()
    assert int(table.support.sum()) == int(count.sum()) and count.sum() >= len(q_of)
    behind = {}
    for b in range(len(q_of)):
        for j in range(count[b]):
            key = (int(batch["relation"][b]),) + tuple(np.stack([rel[b, j], d[b, j]], 1).reshape(-1).tolist())
            behind.setdefault(key, set()).add((int(batch["head"][b]), int(batch["time"][b]), int(objs[b])))
    keys = [tuple(x) for x in table.key().cpu().tolist()]
    assert sorted(behind) == keys
    assert {0, 1, 2} <= set(d[rel != model.n_rel].tolist()) - {-1}              # past, now and future steps all occur
    anchors = np.unique(np.column_stack([batch["head"], batch["time"]]), axis=0)
    q = model.rule_quality(table, anchors=anchors)
    assert isinstance(q, TemporalRuleQuality) and q.table is table and q.n_anchors == len(anchors) and q.hits.is_cuda
    got = torch.stack([q.body_pairs, q.hits, q.pca_body_pairs, q.head_pairs], 1).cpu().numpy()
    low = np.array([len(behind[key]) for key in keys])
    assert (low > 0).all() and (got[:, 0] >= low).all()
    rules = tuple(x.cpu().numpy() for x in (table.head, table.body, table.direction))
    assert np.array_equal(got, T.counts(n_ent, n_rela, n_time, quads, *rules, anchors))
    _invariants(got)
    # the default anchors, and a budget that forces chunks
    full = model.rule_quality(table, scratch_bytes=1 << 16)
    assert full.n_anchors == len(T.default_anchors(quads, n_ent, n_rela))
    got = torch.stack([full.body_pairs, full.hits, full.pca_body_pairs, full.head_pairs], 1).cpu().numpy()
    assert np.array_equal(got, T.counts(n_ent, n_rela, n_time, quads, *rules))
    assert len(full.format()) == len(keys) and (full.confidence() <= 1.0).all()
    # rules_all: the sum of the per-batch tables
    rows = quads[[0, 1, 5, 61, 62, 70, 125, 126, 200, 260]]
    assert (rows[:, 1] != model.n_rel).all()
    parts = None
    for lo in range(0, len(rows), 4):
        part = rows[lo:lo + 4]
        t = model.rules({"head": part[:, 0], "relation": part[:, 1], "time": part[:, 3], "tail": part[:, 2]}, k=2)
        parts = t if parts is None else parts + t
    assert _same_table(model.rules_all(rows, k=2, batch_size=4), parts) and parts.head.numel() > 0
    assert _same_table(model.rules_all(torch.as_tensor(rows), k=2, batch_size=64), parts)
    mined = model.rule_quality(parts)
    assert (mined.confidence()[mined.trivial()] == 1.0).all() and (mined.hits <= mined.body_pairs).all()
    with pytest.raises(ValueError, match="rule_quality: table must be an explain.TemporalRuleTable"):
        model.rule_quality(None)
    with pytest.raises(ValueError, match="rule_quality: the table has n_rel=%d, the model n_rel=%d" % (model.n_rel + 1, model.n_rel)):
        model.rule_quality(TemporalRuleTable(table.head, table.body, table.direction, table.support, table.fixed, model.n_rel + 1))
    with pytest.raises(ValueError, match="rules_all: quads must be"):
        model.rules_all(rows[:, :3])


def _raw(graph, head, body, direc, anchors, n_rules=None, n_hops=None, n_anchors=None):
    """rg_trule_ground itself on sorted anchors int64 [S, 2]: the counts int64 [R, 4] as numpy."""
    from red_gnn_amd import _lib, engine
    dev = torch.device("cuda")
    t32 = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.int32)).to(dev)
    S, R, L = len(anchors), len(head), np.asarray(body).shape[1]
    ptr = np.searchsorted(anchors[:, 1], np.arange(getattr(graph, "n_time", 1) + 1))      # (a static graph, refused, has no n_time)
    h, b, d, e, pt = t32(head), t32(body), t32(direc), t32(anchors[:, 0]), t32(ptr)
    counts = torch.zeros((R, 4), dtype=torch.int64, device=dev)
    scratch = torch.empty(max(engine.trule_ground_scratch_bytes(graph.n_ent, R, S), 4), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().rg_trule_ground(graph.handle, p(h), p(b), p(d), R if n_rules is None else n_rules, L if n_hops is None else n_hops,
                                          p(e), p(pt), S if n_anchors is None else n_anchors, p(scratch), p(counts), _lib.stream_ptr()))
    return counts.cpu().numpy()


def test_errors(case):
    from red_gnn_amd import _lib, engine
    c = case
    tg, r = c["graph"], c["rules"][2]
    sg = engine.Graph(5, 2, np.array([[0, 0, 1], [1, 1, 2], [3, 0, 4]]))
    one = c["default"][:1]
    with pytest.raises(_lib.NativeError, match="rg_trule_ground: static graph"):
        _raw(sg, r[0][:1], r[1][:1], r[2][:1], one)
    dev = torch.device("cuda")
    head, body, src = (torch.zeros(n, dtype=torch.int32, device=dev) for n in (1, 2, 1))
    counts = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    scratch = torch.zeros(engine.rule_ground_scratch_bytes(c["n_ent"], 1, 1), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    with pytest.raises(_lib.NativeError, match="rg_rule_ground: temporal graph"):      # the static entry point still refuses it
        _lib.check(_lib.lib().rg_rule_ground(tg.handle, p(head), p(body), 1, 2, p(src), 1, p(scratch), p(counts), _lib.stream_ptr()))
    with pytest.raises(ValueError, match="rule_ground: temporal graph"):
        engine.rule_ground(tg, np.array([0]), np.array([[0, 1]]))
    for hops in (0, 33):
        with pytest.raises(_lib.NativeError, match="rg_trule_ground: n_hops=%d not in 1..32" % hops):
            _raw(tg, r[0][:1], r[1][:1], r[2][:1], one, n_hops=hops)
    with pytest.raises(_lib.NativeError, match="rg_trule_ground: n_rules=65536 not in"):
        _raw(tg, r[0][:1], r[1][:1], r[2][:1], one, n_rules=65536)
    with pytest.raises(_lib.NativeError, match="rg_trule_ground: n_anchors=-1"):
        _raw(tg, r[0][:1], r[1][:1], r[2][:1], one, n_anchors=-1)
    assert not _raw(tg, r[0][:1], r[1][:1], r[2][:1], one, n_rules=0).any() and not _raw(tg, r[0][:1], r[1][:1], r[2][:1], one, n_anchors=0).any()
    with pytest.raises(ValueError, match="trule_ground: static graph"):
        engine.trule_ground(sg, r[0], r[1], r[2], one)
    bad = r[1].copy()
    bad[0, 1] = c["n_rela"]
    with pytest.raises(ValueError, match=r"trule_ground: relation id out of range 0\.\.%d" % (c["n_rela"] - 1)):
        engine.trule_ground(tg, r[0], bad, r[2])
    with pytest.raises(ValueError, match=r"trule_ground: direction out of range 0\.\.3"):
        engine.trule_ground(tg, r[0], r[1], r[2] + 1)
    with pytest.raises(ValueError, match="trule_ground: duplicate anchors"):
        engine.trule_ground(tg, r[0], r[1], r[2], np.array([[4, 1], [9, 0], [4, 1]]))
    with pytest.raises(ValueError, match="trule_ground: anchor out of range"):
        engine.trule_ground(tg, r[0], r[1], r[2], np.array([[4, c["n_time"]]]))


def test_ids_are_bounded_in_the_kernel(case):
    """The C entry point trusts its caller for the ids (engine.trule_ground validates them): a rule whose step names a relation the
    graph does not have, or a direction that does not exist, grounds nothing, and the other rules of the call are counted as ever."""
    c = case
    head, body, direc = (x.copy() for x in c["rules"][3])
    ref = c["ref_default"][3]
    assert len(head) >= 8 and (ref[:, 0] > 0).sum() >= 4
    body[1, 1], body[3, 0], direc[5, 2] = c["n_rela"], -1, 4
    head[6] = c["n_rela"]                                                          # no such head relation: the body is counted, no head
    got = _raw(c["graph"], head, body, direc, c["default"])
    for i in (1, 3, 5):
        assert got[i, :3].tolist() == [0, 0, 0] and got[i, 3] == ref[i, 3]
    assert got[6].tolist() == [ref[6, 0], 0, 0, 0]
    rest = [i for i in range(len(head)) if i not in (1, 3, 5, 6)]
    assert np.array_equal(got[rest], ref[rest])
