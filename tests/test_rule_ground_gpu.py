"""engine.rule_ground (rg_rule_ground, csrc/rule_ground.hip) and the rule_quality entry points on the MI355X (-m gpu): every count
equal to tests/rule_ground_ref.py on the graph exported from the device - the hand graph of tests/test_rule_ground_ref.py with its
typed-in counts, a synthetic graph with repeated facts under mined and random rules and source sets around the word boundaries, the
smallest chunking, other path lengths, a call whose bitmaps pass 2^31 words, the inductive fixture, BaseModel.rule_quality on family,
the errors, and the kernel's own bound on relation ids."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import rule_ground_ref as R

pytestmark = pytest.mark.gpu


class P:
    def __init__(self, n_layer, hidden_dim, attn_dim, n_rel, act, dropout=0.0):
        self.n_layer, self.hidden_dim, self.attn_dim, self.n_rel, self.act, self.dropout = n_layer, hidden_dim, attn_dim, n_rel, act, dropout


def _opt(loader, n_tbatch):
    class Opt:
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch = 0.01, 0.99, 1e-5, 16, 3, 3, 0.0, "relu", 8
        n_rel = loader.n_rel
    Opt.n_tbatch = n_tbatch
    return Opt


def _rows(graph):
    out_ptr, out_rt, _, _ = graph.export()
    return R.rows_from_export(out_ptr, out_rt)


def _invariants(c):
    assert (c >= 0).all()
    assert (c[:, 1] <= c[:, 2]).all() and (c[:, 2] <= c[:, 0]).all() and (c[:, 1] <= c[:, 3]).all()


def _same_table(a, b):
    a, b = a.cpu(), b.cpu()
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "support", "fixed")) and a.n_rel == b.n_rel


def test_hand_graph():
    from red_gnn_amd import engine
    g = engine.Graph(R.HAND_N_ENT, R.HAND_N_REL, R.HAND_TRIPLES)
    assert np.array_equal(np.unique(_rows(g), axis=0), np.unique(R.hand_rows(), axis=0)) and g.n_fact == len(R.hand_rows())
    got = engine.rule_ground(g, R.HAND_HEAD, R.HAND_BODY)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (5, 4)
    assert np.array_equal(got.cpu().numpy(), R.HAND_ALL)
    assert np.array_equal(engine.rule_ground(g, torch.as_tensor(R.HAND_HEAD).cuda(), torch.as_tensor(R.HAND_BODY).cuda(),
                                             torch.as_tensor(R.HAND_SOURCES, dtype=torch.int32)).cpu().numpy(), R.HAND_SUB)
    empty = engine.rule_ground(g, R.HAND_HEAD[:0], R.HAND_BODY[:0])
    assert empty.is_cuda and empty.shape == (0, 4) and empty.dtype == torch.int64
    assert not engine.rule_ground(g, R.HAND_HEAD, R.HAND_BODY, np.zeros(0, np.int64)).any()


SOURCE_SIZES = (None, 1, 31, 33, 65)


@pytest.fixture(scope="module")
def synthetic():
    """The graph (about 50 facts stated twice), the rules - the k = 4 table of 24 test rows and 40 random bodies of length 3 over
    0..2*n_rel, identity and inverse ids among them - the source sets, and the reference counts of each, computed once."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(300, 7, 3000, seed=3)
    facts = np.concatenate([kg.facts, kg.facts[:50]], 0)
    loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=facts, train=kg.train, valid=kg.valid, test=kg.test),
                        verbose=False)
    torch.manual_seed(1234)
    model = RED_GNN_trans(P(3, 16, 5, loader.n_rel, "relu"), loader).cuda().eval()
    test = np.asarray(kg.test)[:24].astype(np.int64)
    table = model.rules(test[:, 0], test[:, 1], test[:, 2], k=4)
    n_rela = 2 * kg.n_rel + 1
    rng = np.random.default_rng(5)
    body40, head40 = rng.integers(0, n_rela, (40, 3)), rng.integers(0, n_rela, 40)
    assert (body40 == n_rela - 1).any() and ((body40 >= kg.n_rel) & (body40 < n_rela - 1)).any()
    ident = n_rela - 1                                                         # ... and the trivial rule of relation 2, twice
    head = np.concatenate([table.head.cpu().numpy(), head40, [2, 2]])
    body = np.concatenate([table.body.cpu().numpy(), body40, [[ident, ident, 2], [2, ident, ident]]], 0)
    graph = loader.graph_for("test")
    rows = _rows(graph)
    assert len(rows) > len(np.unique(rows, axis=0))                            # the repeated facts are in the device graph
    sources = {n: None if n is None else rng.permutation(kg.n_ent)[:n] for n in SOURCE_SIZES}
    ref = {n: R.counts(kg.n_ent, n_rela, rows, head, body, s) for n, s in sources.items()}
    return dict(model=model, table=table, graph=graph, rows=rows, n_ent=kg.n_ent, n_rel=kg.n_rel, n_rela=n_rela, head=head, body=body,
                sources=sources, ref=ref)


@pytest.mark.parametrize("n_sources", SOURCE_SIZES)
def test_synthetic_counts_equal_the_reference(synthetic, n_sources):
    from red_gnn_amd import engine
    s = synthetic
    got = engine.rule_ground(s["graph"], s["head"], s["body"], s["sources"][n_sources]).cpu().numpy()
    ref = s["ref"][n_sources]
    assert got.shape == ref.shape == (len(s["head"]), 4) and len(s["head"]) > 40
    assert np.array_equal(got, ref)
    _invariants(got)
    if n_sources == 33:                      # the definition itself, where the n_ent^3 products are cheap: 33 rows
        assert np.array_equal(got, R.counts_dense(s["n_ent"], s["n_rela"], s["rows"], s["head"], s["body"], s["sources"][33]))


def test_synthetic_comparison_is_not_vacuous(synthetic):
    """Every relation of this graph has hundreds of facts, so over all 300 sources every length-3 body connects something: the rule
    without a grounding is looked for where it exists, in the run from a single source."""
    s = synthetic
    step = s["body"] != s["n_rela"] - 1
    trivial = (step.sum(1) == 1) & ((s["body"] * step).sum(1) == s["head"])
    every = s["ref"][None]
    assert ((every[:, 1] > 0) & (every[:, 1] < every[:, 0]) & ~trivial).any()
    one = s["ref"][1]
    assert (one[:, 0] == 0).any() and (one[:, 0] > 0).any() and (one[:, 3] == 0).any() and (one[:, 3] > 0).any()
    assert trivial[-2:].all() and (every[trivial, 0] == every[trivial, 1]).all() and (every[trivial, 0] == every[trivial, 3]).all()
    assert (every[trivial, 0] > 0).all()


def test_chunking_changes_no_bit(synthetic):
    from red_gnn_amd import engine
    s = synthetic
    small = engine.rule_ground_scratch_bytes(s["n_ent"], 1, 32)
    assert engine.rule_chunking(s["n_ent"], len(s["head"]), s["n_ent"], small) == (1, 32)
    whole = engine.rule_ground(s["graph"], s["head"], s["body"])
    assert torch.equal(engine.rule_ground(s["graph"], s["head"], s["body"], scratch_bytes=small), whole)
    src = s["sources"][65]
    assert torch.equal(engine.rule_ground(s["graph"], s["head"], s["body"], src, scratch_bytes=small),
                       engine.rule_ground(s["graph"], s["head"], s["body"], src))
    mid = engine.rule_ground_scratch_bytes(s["n_ent"], 7, 96)                  # 7 rules x 96 sources
    assert torch.equal(engine.rule_ground(s["graph"], s["head"], s["body"], scratch_bytes=mid), whole)
    assert np.array_equal(whole.cpu().numpy(), s["ref"][None])


@pytest.mark.parametrize("L", [1, 5])
def test_other_path_lengths(synthetic, L):
    from red_gnn_amd import engine
    s = synthetic
    rng = np.random.default_rng(100 + L)
    head, body = rng.integers(0, s["n_rela"], 30), rng.integers(0, s["n_rela"], (30, L))
    for src in (None, s["sources"][33]):
        got = engine.rule_ground(s["graph"], head, body, src).cpu().numpy()
        assert np.array_equal(got, R.counts(s["n_ent"], s["n_rela"], s["rows"], head, body, src))
        _invariants(got)
        assert (got[:, 0] > 0).any()


def test_word_indices_past_2_31():
    """17 rules x 66 001 entities x 2063 words are 2.31 G words per bitmap (27.8 GB of scratch in one chunk): the last rule's rows lie
    wholly beyond word 2^31 and the one before crosses it.  The graph has 160 facts among its first and last 20 entities, so the
    reference is a handful of sparse products; id ^ id -> id sets one bit in every row of the bitmap beyond 2^31."""
    from red_gnn_amd import engine
    n_ent, n_rel, n_rela, trip = R.wide_graph(66001)
    head, body = R.wide_rules(n_rela)
    W = (n_ent + 31) // 32
    assert (len(head) - 1) * n_ent * W > 2 ** 31
    budget = 32 << 30
    assert engine.rule_chunking(n_ent, len(head), n_ent, budget) == (len(head), 32 * W)
    g = engine.Graph(n_ent, n_rel, trip)
    got = engine.rule_ground(g, head, body, scratch_bytes=budget).cpu().numpy()
    ref = R.counts_sparse(n_ent, n_rela, _rows(g), head, body)
    assert np.array_equal(got, ref)
    assert ref[-2].tolist() == [n_ent] * 4 and 0 < ref[-1, 1] < ref[-1, 2] < ref[-1, 0]
    assert np.array_equal(engine.rule_ground(g, head, body).cpu().numpy(), ref)       # the default budget: a rule and 2/3 of the sources per chunk
    del g
    torch.cuda.empty_cache()                                                     # the 27.8 GB go back before the next test


def test_model_rule_quality(synthetic):
    s = synthetic
    q = s["model"].rule_quality(s["table"])
    n = s["table"].head.numel()
    ref = s["ref"][None][:n]
    assert q.table is s["table"] and q.n_sources == s["n_ent"] and q.hits.is_cuda
    got = torch.stack([q.body_pairs, q.hits, q.pca_body_pairs, q.head_pairs], 1).cpu().numpy()
    assert np.array_equal(got, ref)
    assert np.array_equal(q.confidence().cpu().numpy(), np.where(ref[:, 0] > 0, ref[:, 1] / np.maximum(ref[:, 0], 1), 0.0))
    src = s["sources"][31]
    q31 = s["model"].rule_quality(s["table"], sources=src, scratch_bytes=1 << 16)
    assert q31.n_sources == 31 and np.array_equal(q31.hits.cpu().numpy(), s["ref"][31][:n, 1])
    assert len(q.format()) == n and q.top(int(s["table"].head[0]), 3, min_hits=0, drop_trivial=False).numel() >= 1


def test_inductive():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    loader = DataLoader(ids=U.load("ind_WN18RR_v1_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 32), loader)
    assert isinstance(bm.model, RED_GNN_induc)
    table = bm.rules("test", k=2, max_queries=60)
    n_rela = 2 * loader.n_rel + 1
    for mode, kw in (("inductive", dict(mode="inductive")), ("transductive", {})):      # the model's default is the training graph
        graph = loader.graph_for(mode)
        q = bm.model.rule_quality(table, **kw)
        assert q.n_sources == graph.n_ent
        ref = R.counts(graph.n_ent, n_rela, _rows(graph), table.head.cpu().numpy(), table.body.cpu().numpy())
        got = torch.stack([q.body_pairs, q.hits, q.pca_body_pairs, q.head_pairs], 1).cpu().numpy()
        assert np.array_equal(got, ref) and (ref[:, 0] > 0).any()
        _invariants(got)
    assert loader.graph_for("inductive").n_ent != loader.graph_for("transductive").n_ent
    qb = bm.rule_quality(table, "test")                                         # the test split is scored on the inductive graph
    assert torch.equal(qb.hits, bm.model.rule_quality(table, mode="inductive").hits)


def test_base_model_rule_quality_family():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    loader = DataLoader(ids=U.load("family_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 64), loader)
    q = bm.rule_quality(data="test", k=2, max_queries=100)
    table = bm.rules("test", k=2, max_queries=100)
    assert _same_table(q.table, table) and table.head.numel() > 0
    graph = loader.graph_for("test")
    ref = R.counts(graph.n_ent, 2 * loader.n_rel + 1, _rows(graph), table.head.cpu().numpy(), table.body.cpu().numpy())
    got = torch.stack([q.body_pairs, q.hits, q.pca_body_pairs, q.head_pairs], 1).cpu().numpy()
    assert np.array_equal(got, ref)
    _invariants(got)
    assert q.n_sources == graph.n_ent
    trivial = q.trivial().cpu().numpy()
    conf = q.confidence().cpu().numpy()
    assert (conf[trivial] == 1.0).all()
    assert ((conf >= 0.0) & (conf <= 1.0)).all() and (q.pca_confidence() >= q.confidence()).all()
    with pytest.raises(ValueError, match="rule_quality: data must be 'valid' or 'test'"):
        bm.rule_quality(table, "train")


def test_errors(synthetic):
    from red_gnn_amd import _lib, engine
    from red_gnn_amd.explain import RuleTable
    s = synthetic
    quads = np.array([[0, 0, 1, 0], [1, 1, 2, 1], [2, 0, 0, 1], [0, 2, 0, 0], [1, 2, 1, 0], [2, 2, 2, 0]], dtype=np.int32)
    tg = engine.TemporalGraph(3, 3, 2, quads)
    with pytest.raises(ValueError, match="rule_ground: temporal graph"):
        engine.rule_ground(tg, np.array([0]), np.array([[0, 1]]))
    dev = torch.device("cuda")
    head, body, src = (torch.zeros(n, dtype=torch.int32, device=dev) for n in (1, 2, 1))
    counts = torch.zeros((1, 4), dtype=torch.int64, device=dev)
    scratch = torch.zeros(engine.rule_ground_scratch_bytes(3, 1, 1), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    with pytest.raises(_lib.NativeError, match="rg_rule_ground: temporal graph"):      # the C entry point's own check, before any launch
        _lib.check(_lib.lib().rg_rule_ground(tg.handle, p(head), p(body), 1, 2, p(src), 1, p(scratch), p(counts), _lib.stream_ptr()))
    for hops in (0, 33):
        with pytest.raises(_lib.NativeError, match="rg_rule_ground: n_hops=%d not in 1..32" % hops):
            _lib.check(_lib.lib().rg_rule_ground(s["graph"].handle, p(head), p(body), 1, hops, p(src), 1, p(scratch), p(counts),
                                                 _lib.stream_ptr()))
    with pytest.raises(_lib.NativeError, match="rg_rule_ground: n_rules=65536 not in"):
        _lib.check(_lib.lib().rg_rule_ground(s["graph"].handle, p(head), p(body), 65536, 2, p(src), 1, p(scratch), p(counts),
                                             _lib.stream_ptr()))
    assert not counts.any()
    bad = s["body"][:1].copy()
    bad[0, 1] = s["n_rela"]
    with pytest.raises(ValueError, match=r"rule_ground: relation id out of range 0\.\.%d" % (s["n_rela"] - 1)):
        engine.rule_ground(s["graph"], s["head"][:1], bad)
    with pytest.raises(ValueError, match="rule_ground: duplicate sources"):
        engine.rule_ground(s["graph"], s["head"], s["body"], np.array([4, 9, 4]))
    t = s["table"]
    with pytest.raises(ValueError, match="rule_quality: the table has n_rel=%d, the model n_rel=%d" % (s["n_rel"] + 1, s["n_rel"])):
        s["model"].rule_quality(RuleTable(t.head, t.body, t.support, t.fixed, s["n_rel"] + 1))


def test_relation_ids_are_bounded_in_the_kernel(synthetic):
    """The C entry point trusts its caller for the ids (engine.rule_ground validates them); a rule whose head or body names a
    relation the graph does not have grounds nothing, and the other rules of the call are counted as ever."""
    from red_gnn_amd import _lib, engine
    s = synthetic
    g, dev, n = s["graph"], torch.device("cuda"), s["n_ent"]
    head = torch.tensor([s["n_rela"], 0, 0, int(s["head"][0])], dtype=torch.int32, device=dev)
    body = torch.tensor([[0, 1, 2], [0, -1, 2], [0, 1, 2 ** 31 - 1], s["body"][0].tolist()], dtype=torch.int32, device=dev)
    src = torch.arange(n, dtype=torch.int32, device=dev)
    counts = torch.zeros((4, 4), dtype=torch.int64, device=dev)
    scratch = torch.empty(engine.rule_ground_scratch_bytes(n, 4, n), dtype=torch.uint8, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().rg_rule_ground(g.handle, p(head), p(body), 4, 3, p(src), n, p(scratch), p(counts), _lib.stream_ptr()))
    got = counts.cpu().numpy()
    ref = s["ref"][None]
    assert got[0, 3] == 0 and got[0, 1] == 0 and got[0, 0] > 0                  # no such head relation
    assert got[1, 0] == 0 and got[2, 0] == 0 and got[1, 3] == got[2, 3] > 0     # no such step
    assert np.array_equal(got[3], ref[0])
