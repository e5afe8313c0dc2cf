"""engine.rule_apply (rg_rule_apply, csrc/rule_apply.hip), model.rule_scores / rule_predict and BaseModel.rule_evaluate on the MI355X
(-m gpu): every output equal bit for bit to tests/rule_apply_ref.py on the graph exported from the device - the hand graph with its
typed-in cells, a synthetic graph with repeated facts under mined and random rules and per-relation query counts around the word
boundaries, the smallest chunking, other path lengths, slabs past 2^31 words, the model entry points, the split evaluation on family
and the inductive fixture, the errors, and the kernel's own bound on relation ids."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import rank_ref
from tests import rule_apply_ref as A
from tests import rule_ground_ref as G

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
    return G.rows_from_export(out_ptr, out_rt)


def _np(four):
    return tuple(t.cpu().numpy() for t in four)


def _check_types(four, B, n_ent):
    assert all(t.is_cuda and t.shape == (B, n_ent) for t in four)
    assert [t.dtype for t in four] == [torch.float32, torch.float32, torch.int32, torch.int32]


def test_hand_graph():
    from red_gnn_amd import engine
    g = engine.Graph(G.HAND_N_ENT, G.HAND_N_REL, G.HAND_TRIPLES)
    got = engine.rule_apply(g, A.HAND_HEAD, A.HAND_BODY, A.HAND_WEIGHT, A.HAND_SUBS, A.HAND_RELS)
    _check_types(got, len(A.HAND_SUBS), G.HAND_N_ENT)
    assert A.same(_np(got), A.hand_expected())
    as_t = lambda a: torch.as_tensor(a).cuda()
    again = engine.rule_apply(g, as_t(A.HAND_HEAD), as_t(A.HAND_BODY), as_t(A.HAND_WEIGHT), as_t(A.HAND_SUBS), as_t(A.HAND_RELS))
    assert A.same(_np(again), A.hand_expected())
    none = engine.rule_apply(g, A.HAND_HEAD[:0], A.HAND_BODY[:0], A.HAND_WEIGHT[:0], A.HAND_SUBS, A.HAND_RELS)       # R = 0
    _check_types(none, len(A.HAND_SUBS), G.HAND_N_ENT)
    assert A.same(_np(none), A.initial(len(A.HAND_SUBS), G.HAND_N_ENT))
    empty = engine.rule_apply(g, A.HAND_HEAD, A.HAND_BODY, A.HAND_WEIGHT, A.HAND_SUBS[:0], A.HAND_RELS[:0])         # B = 0
    _check_types(empty, 0, G.HAND_N_ENT)
    only = engine.rule_apply(g, A.HAND_HEAD, A.HAND_BODY, A.HAND_WEIGHT, A.HAND_SUBS[6:], A.HAND_RELS[6:])          # no rule has a query
    assert A.same(_np(only), A.initial(1, G.HAND_N_ENT))


QUERY_COUNTS = (65, 33, 32, 31, 1, 0)


@pytest.fixture(scope="module")
def synthetic():
    """The graph of tests/test_rule_ground_gpu.py (50 facts stated twice), rebuilt here; the rules - the k = 4 table of 24 test rows
    and 60 random bodies of length 3 over 0..2*n_rel, identity and inverse ids among them - sorted by (head, body) and weighted
    hits / (body_pairs + 5) from the reference counts (a rule without a hit has weight 0 and is left out, as rule_scores leaves it
    out); the queries, and the reference outputs, computed once."""
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
    rng = np.random.default_rng(11)
    body60, head60 = rng.integers(0, n_rela, (60, 3)), rng.integers(0, n_rela, 60)
    assert (body60 == n_rela - 1).any() and ((body60 >= kg.n_rel) & (body60 < n_rela - 1)).any()
    key = np.unique(np.concatenate([np.concatenate([table.head.cpu().numpy()[:, None], table.body.cpu().numpy()], 1),
                                    np.concatenate([head60[:, None], body60], 1)], 0), axis=0)             # sorted by (head, body)
    graph = loader.graph_for("test")
    rows = _rows(graph)
    assert len(rows) > len(np.unique(rows, axis=0))                            # the repeated facts are in the device graph
    counts = G.counts(kg.n_ent, n_rela, rows, key[:, 0], key[:, 1:])
    weight = (counts[:, 1] / (counts[:, 0] + 5.0)).astype(np.float32)
    rel_ids = np.unique(key[weight > 0, 0])
    assert len(rel_ids) >= len(QUERY_COUNTS) + 1
    no_rule = int(rel_ids[-1])                                                 # this relation keeps its queries and loses its rules
    keep = (weight > 0) & (key[:, 0] != no_rule)
    head, body, weight = key[keep, 0], key[keep, 1:], weight[keep]
    assert len(head) >= 60 and (weight <= 1).all()
    n_of = dict(zip(rel_ids[:len(QUERY_COUNTS)].tolist(), QUERY_COUNTS))
    n_of[no_rule] = 3
    rels = np.concatenate([np.full(n, r) for r, n in n_of.items()])
    subs = rng.integers(0, kg.n_ent, len(rels))
    subs[1] = subs[0]                                                          # a query stated twice (rels[0] == rels[1])
    mix = rng.permutation(len(rels))
    subs, rels = subs[mix], rels[mix]
    ref = A.apply_dense(kg.n_ent, n_rela, rows, head, body, weight, subs, rels)
    return dict(model=model, loader=loader, table=table, graph=graph, rows=rows, n_ent=kg.n_ent, n_rel=kg.n_rel, n_rela=n_rela,
                head=head, body=body, weight=weight, subs=subs, rels=rels, ref=ref, n_of=n_of, no_rule=no_rule, kg=kg)


def test_synthetic_equals_the_reference(synthetic):
    from red_gnn_amd import engine
    s = synthetic
    got = engine.rule_apply(s["graph"], s["head"], s["body"], s["weight"], s["subs"], s["rels"])
    _check_types(got, len(s["subs"]), s["n_ent"])
    assert A.same(_np(got), s["ref"])
    assert np.array_equal((1.0 - got[1]).cpu().numpy().view(np.int32), A.scores(*s["ref"][:2], "noisy_or").view(np.int32))


def test_synthetic_comparison_is_not_vacuous(synthetic):
    s = synthetic
    best, surv, rule, fired = s["ref"]
    assert sorted(np.bincount(s["rels"], minlength=s["n_rela"])[list(s["n_of"])].tolist()) == sorted(QUERY_COUNTS + (3,))
    assert (fired >= 2).any() and (fired == 0).any()
    mx, nor = A.scores(best, surv, "max"), A.scores(best, surv, "noisy_or")
    assert any(not np.array_equal(A.order(mx[b]), A.order(nor[b])) for b in range(len(mx)))               # a row the two rank differently
    empty_pair = False                                                         # a (query, rule of its relation) pair that reaches nothing
    first = np.full(fired.shape, -1)                                           # the first rule that fires per cell
    for i in range(len(s["head"])):
        one = A.apply_dense(s["n_ent"], s["n_rela"], s["rows"], s["head"][i:i + 1], s["body"][i:i + 1], s["weight"][i:i + 1],
                            s["subs"], s["rels"])[3]
        mine = s["rels"] == s["head"][i]
        empty_pair |= bool(mine.any() and (one[mine].sum(1) == 0).any())
        first[(one > 0) & (first < 0)] = i
    assert empty_pair
    assert ((rule != first) & (fired >= 2)).any() and ((rule == first) & (fired >= 2)).any()              # a later, larger weight displaced one
    zero = [r for r, n in s["n_of"].items() if n == 0][0]
    assert (s["head"] == zero).any()                                            # a rule without a query
    assert not (s["head"] == s["no_rule"]).any() and (s["rels"] == s["no_rule"]).sum() == 3                # queries without a rule
    assert not fired[s["rels"] == s["no_rule"]].any()
    assert len(np.unique(np.stack([s["subs"], s["rels"]], 1), axis=0)) < len(s["subs"])                   # a duplicate query


def test_chunking_changes_no_bit(synthetic):
    from red_gnn_amd import engine
    s = synthetic
    R = len(s["head"])
    counts = np.bincount(s["rels"], minlength=s["n_rela"])
    words = s["n_ent"] * ((counts[s["head"]] + 31) // 32)
    assert engine.rule_apply_chunking(words, engine.RULE_SCRATCH_BYTES) == [(0, R)]
    assert engine.rule_apply_chunking(words, 0) == [(i, i + 1) for i in range(R)] and len(np.unique(s["head"])) < R
    for n in (1, 64, 65, int(words.sum())):
        assert engine.rule_apply_scratch_bytes(n) == engine._lib.lib().rg_rule_apply_scratch_bytes(n)
    args = (s["graph"], s["head"], s["body"], s["weight"], s["subs"], s["rels"])
    whole = engine.rule_apply(*args)
    one = engine.rule_apply(*args, scratch_bytes=0)                              # one rule per call: every head's rules are cut apart
    mid = engine.rule_apply(*args, scratch_bytes=engine.rule_apply_scratch_bytes(int(words[:7].sum())))
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(whole, one, mid))
    assert A.same(_np(whole), s["ref"])


@pytest.mark.parametrize("L", [1, 2, 4])
def test_path_lengths(synthetic, L):
    from red_gnn_amd import engine
    s = synthetic
    rng = np.random.default_rng(200 + L)
    head, body = np.sort(rng.integers(0, s["n_rela"], 30)), rng.integers(0, s["n_rela"], (30, L))
    weight = rng.integers(1, 257, 30).astype(np.float32) / np.float32(256)
    got = engine.rule_apply(s["graph"], head, body, weight, s["subs"], s["rels"])
    ref = A.apply_dense(s["n_ent"], s["n_rela"], s["rows"], head, body, weight, s["subs"], s["rels"])
    assert A.same(_np(got), ref)
    assert (ref[3] > 0).any() and (ref[3] == 0).any()


def test_slab_words_past_2_31():
    """520 rules of one head x 66 001 entities x 65 words (2080 queries of that relation) are 2.23 G words per bitmap region (17.8 GB
    of scratch in one call, 2.2 GB of outputs): the slabs of the last 19 rules lie wholly beyond word 2^31 and rule 500 crosses it.  The
    graph has 160 facts among its first and last 20 entities, so the reference is a handful of sparse products; the expected tensors
    are scattered on the device."""
    from red_gnn_amd import engine
    n_ent, n_rel, n_rela, trip = G.wide_graph(66001)
    rng = np.random.default_rng(12)
    R, B, h = 520, 2080, 1
    head, body = np.full(R, h), rng.integers(0, n_rela, (R, 2))
    body[-1], body[-2], body[-3], body[500] = (n_rela - 1, n_rela - 1), (0, 1), (n_rela - 1, 0), (1, 3)
    weight = rng.integers(1, 1024, R).astype(np.float32) / np.float32(1024)
    weight[-1] = 1.0                                                             # id ^ id, the last rule, is the best of every (b, sub[b])
    pool = np.concatenate([np.arange(20), np.arange(n_ent - 20, n_ent)])
    subs = np.concatenate([pool, pool[:8], rng.integers(0, n_ent, B - 48)])
    rels = np.full(B, h)
    W = (B + 31) // 32
    assert W == 65 and 501 * n_ent * W > 2 ** 31 > 500 * n_ent * W
    budget = 20 << 30
    assert engine.rule_apply_chunking(np.full(R, n_ent * W), budget) == [(0, R)]
    g = engine.Graph(n_ent, n_rel, trip)
    cells = A.apply_cells(n_ent, n_rela, _rows(g), head, body, weight, subs, rels)
    b, y, best, surv, rule, fired = A.cells_arrays(cells, n_ent)
    assert (rule >= 501).any() and (fired >= 2).any() and (rule == R - 1).any() and len(b) > B
    got = engine.rule_apply(g, head, body, weight, subs, rels, scratch_bytes=budget)
    dev = got[0].device
    at = (torch.as_tensor(b).to(dev), torch.as_tensor(y).to(dev))
    for t, fill, vals in zip(got, (0.0, 1.0, -1, 0), (best, surv, rule, fired)):
        exp = torch.full_like(t, fill)
        exp[at] = torch.as_tensor(vals).to(dev)
        assert torch.equal(t, exp)
        del exp
    del got, g
    torch.cuda.empty_cache()                                                     # the 20 GB go back before the next test


def _ref_quality_weights(s, table, laplace, by_pca=False):
    """(rows kept, weights) of model.rule_scores restated from the reference counts."""
    head, body = table.head.cpu().numpy(), table.body.cpu().numpy()
    c = G.counts(s["n_ent"], s["n_rela"], s["rows"], head, body)
    den = c[:, 2 if by_pca else 0] + float(laplace)
    w = np.where(den > 0, c[:, 1] / np.where(den > 0, den, 1.0), 0.0).astype(np.float32)
    step = body != s["n_rela"] - 1
    trivial = (step.sum(1) == 1) & ((body * step).sum(1) == head)
    return c, w, trivial


def test_model_rule_scores_and_predict(synthetic):
    from red_gnn_amd.explain import RulePrediction, RuleScores
    s = synthetic
    model, table, n_ent = s["model"], s["table"], s["n_ent"]
    quality = model.rule_quality(table)
    test = np.asarray(s["kg"].test)[:40].astype(np.int64)
    subs, rels = test[:, 0], test[:, 1]
    head, body = table.head.cpu().numpy(), table.body.cpu().numpy()
    many = int(np.median(G.counts(n_ent, s["n_rela"], s["rows"], head, body)[:, 1])) + 1              # hits of more than half the rules are below
    for kw, laplace, pca in ((dict(laplace=5.0), 5.0, False), (dict(by="pca_confidence", min_hits=many), 0.0, True)):
        c, w, trivial = _ref_quality_weights(s, table, laplace, pca)
        rows = np.nonzero((c[:, 1] >= kw.get("min_hits", 1)) & (w > 0) & ~trivial)[0]
        assert 0 < len(rows) <= len(head) and (pca is False or len(rows) < len(head))
        ref = A.apply_dense(n_ent, s["n_rela"], s["rows"], head[rows], body[rows], w[rows], subs, rels)
        rs = model.rule_scores(quality, subs, rels, **kw)
        assert isinstance(rs, RuleScores) and np.array_equal(rs.rows.cpu().numpy(), rows)
        exp_rule = np.where(ref[2] >= 0, rows[np.maximum(ref[2], 0)], -1).astype(np.int32)
        assert A.same(_np((rs.best, rs.surv, rs.best_rule, rs.fired)), (ref[0], ref[1], exp_rule, ref[3]))
        assert np.array_equal(rs.covered().cpu().numpy(), ref[3] > 0) and (ref[3] > 0).any()
        keys, ptr, idx = s["loader"].known_index("test")
        for agg, exclude in (("noisy_or", True), ("max", True), ("noisy_or", False)):
            k = 7
            pred = model.rule_predict(quality, subs, rels, k=k, agg=agg, exclude_known=exclude, **kw)
            assert isinstance(pred, RulePrediction)
            assert [t.dtype for t in (pred.ids, pred.scores, pred.rule, pred.fired)] == [torch.int64, torch.float32, torch.int64, torch.int32]
            assert all(t.shape == (len(subs), k) and t.is_cuda for t in (pred.ids, pred.scores, pred.rule, pred.fired))
            sc = A.scores(ref[0], ref[1], agg)
            dropped = 0
            for b in range(len(subs)):
                at = np.searchsorted(keys, subs[b] * s["n_rela"] + rels[b])
                known = idx[ptr[at]:ptr[at + 1]] if exclude and at < len(keys) and keys[at] == subs[b] * s["n_rela"] + rels[b] else []
                dropped += len(known)
                top = A.order(sc[b], known)[:k]
                assert np.array_equal(pred.ids[b].cpu().numpy(), top)
                assert np.array_equal(pred.scores[b].cpu().numpy().view(np.int32), sc[b, top].view(np.int32))
                assert np.array_equal(pred.rule[b].cpu().numpy(), exp_rule[b, top])
                assert np.array_equal(pred.fired[b].cpu().numpy(), ref[3][b, top])
            assert dropped > 0 or not exclude
            assert len(pred.format()) == len(subs) * k
    lines = pred.format(id2rel=["rel%d" % i for i in range(s["n_rel"])])
    assert any("rel" in ln and "->" in ln for ln in lines) and all(ln.startswith("row ") for ln in lines)


def test_predict_past_the_end_and_the_trivial_rule(synthetic):
    """k beyond the entities that remain gives -1 / -inf / -1 / 0; the trivial rule alone, with drop_trivial=False, fires exactly on
    the graph's adjacency of each (s, r)."""
    from red_gnn_amd import engine
    from red_gnn_amd.explain import RuleQuality, RuleTable
    s = synthetic
    model, n_ent, ident = s["model"], s["n_ent"], s["n_rela"] - 1
    dev = torch.device("cuda")
    head = torch.arange(s["n_rel"], dtype=torch.int64, device=dev)
    body = torch.stack([torch.full_like(head, ident), head, torch.full_like(head, ident)], 1)
    one = torch.ones_like(head)
    table = RuleTable(head, body, one, one.clone(), s["n_rel"])
    quality = model.rule_quality(table)
    assert isinstance(quality, RuleQuality) and bool(quality.trivial().all()) and bool((quality.confidence() == 1).all())
    test = np.asarray(s["kg"].test)[:30].astype(np.int64)
    subs, rels = test[:, 0], test[:, 1]
    assert not model.rule_scores(quality, subs, rels).fired.any() and model.rule_scores(quality, subs, rels).rows.numel() == 0
    rs = model.rule_scores(quality, subs, rels, drop_trivial=False)
    adj = np.zeros((len(subs), n_ent), np.int32)
    for b in range(len(subs)):
        adj[b, s["rows"][(s["rows"][:, 0] == subs[b]) & (s["rows"][:, 1] == rels[b]), 2]] = 1
    assert np.array_equal(rs.fired.cpu().numpy(), adj) and adj.any()
    assert np.array_equal(rs.best.cpu().numpy(), adj.astype(np.float32)) and np.array_equal(rs.best_rule.cpu().numpy(), np.where(adj > 0, rels[:, None], -1))
    k = n_ent
    pred = model.rule_predict(quality, subs, rels, k=k, drop_trivial=False)
    ids = pred.ids.cpu().numpy()
    assert (ids[:, -1] == -1).all()                                              # the test answer itself is a known tail
    past = ids < 0
    assert np.isneginf(pred.scores.cpu().numpy()[past]).all() and (pred.rule.cpu().numpy()[past] == -1).all()
    assert (pred.fired.cpu().numpy()[past] == 0).all() and (pred.fired.cpu().numpy()[~past] == 0).all()  # every adjacent tail is known
    del engine


def _ref_split(loader, graph, quality, data, n_q, agg):
    """(ranks in (query, ascending answer) order, answers some rule reaches) of the rule scores by the references."""
    rows = _rows(graph)
    n_rela = 2 * loader.n_rel + 1
    q = quality.cpu()
    head, body = q.table.head.numpy(), q.table.body.numpy()
    w = np.where(q.body_pairs.numpy() > 0, q.hits.numpy() / np.maximum(q.body_pairs.numpy(), 1), 0.0).astype(np.float32)
    step = body != n_rela - 1
    trivial = (step.sum(1) == 1) & ((body * step).sum(1) == head)
    keep = np.nonzero((q.hits.numpy() >= 1) & (w > 0) & ~trivial)[0]
    subs, rels, ap, ai, fp, fi = loader.get_batch_csr(np.arange(n_q), data=data)
    subs, rels = np.asarray(subs), np.asarray(rels)
    ap, ai, fp, fi = (t.cpu().numpy() for t in (ap, ai, fp, fi))
    cells = A.apply_cells(graph.n_ent, n_rela, rows, head[keep], body[keep], w[keep], subs, rels)
    best, surv, rule, fired = A.cells_to_dense(cells, n_q, graph.n_ent)
    ranks = rank_ref.ranks(A.scores(best, surv, agg), ap, ai, fp, fi)
    covered = sum(int(fired[b, ai[i]] > 0) for b in range(n_q) for i in range(ap[b], ap[b + 1]))
    return ranks, covered, len(keep)


def _same_table(a, b):
    a, b = a.cpu(), b.cpu()
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "support", "fixed")) and a.n_rel == b.n_rel


def _check_rule_evaluate(bm, loader, n_q, mine_mode):
    from red_gnn_amd.explain import split_rule_ranks
    from red_gnn_amd.utils import cal_performance
    quality = bm.rule_quality(data="valid", k=1, max_queries=n_q)
    assert _same_table(quality.table, bm.rules("valid", k=1, max_queries=n_q))
    assert torch.equal(quality.hits, bm.model.rule_quality(quality.table, mode=mine_mode).hits)           # counted where valid is scored
    graph = loader.graph_for(loader.eval_mode("test") if hasattr(loader, "eval_mode") else "test")
    for agg, batch in (("noisy_or", 256), ("max", 37)):
        ref_ranks, ref_cov, n_keep = _ref_split(loader, graph, quality, "test", n_q, agg)
        assert n_keep > 0 and 0 < ref_cov
        ranks, covered = split_rule_ranks(bm, quality, "test", agg, batch, n_q)
        assert ranks.dtype == torch.float64 and np.array_equal(ranks.cpu().numpy(), ref_ranks) and covered == ref_cov
        out = bm.rule_evaluate(quality, data="test", agg=agg, batch=batch, max_queries=n_q)
        mrr, h1, h10 = cal_performance(ref_ranks)
        assert out == dict(mrr=float(mrr), h1=float(h1), h10=float(h10), n=len(ref_ranks), coverage=ref_cov / len(ref_ranks))
    default = bm.rule_evaluate(max_queries=n_q)                                  # mines on valid, scores test, noisy-or
    ref_ranks, ref_cov, _ = _ref_split(loader, graph, quality, "test", n_q, "noisy_or")
    assert default["n"] == len(ref_ranks) and default["coverage"] == ref_cov / len(ref_ranks)
    assert default["mrr"] == float(cal_performance(ref_ranks)[0])
    return quality


def test_rule_evaluate_family():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    loader = DataLoader(ids=U.load("family_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 64), loader)
    quality = _check_rule_evaluate(bm, loader, 100, "valid")
    for kw, match in ((dict(data="train"), "rule_evaluate: data must be 'valid' or 'test'"),
                      (dict(mine="train"), "rule_evaluate: mine must be 'valid' or 'test'"),
                      (dict(agg="sum"), "rule_evaluate: agg must be 'noisy_or' or 'max'"),
                      (dict(batch=0), "rule_evaluate: batch must be a positive integer")):
        with pytest.raises(ValueError, match=match):
            bm.rule_evaluate(quality, max_queries=10, **kw)


def test_rule_evaluate_inductive():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    loader = DataLoader(ids=U.load("ind_WN18RR_v1_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 32), loader)
    assert isinstance(bm.model, RED_GNN_induc)
    _check_rule_evaluate(bm, loader, 60, "transductive")                         # mined and counted on the training graph,
    assert loader.graph_for("inductive").n_ent != loader.graph_for("transductive").n_ent                  # applied on the inductive one


def test_errors(synthetic):
    from red_gnn_amd import _lib, engine
    from red_gnn_amd.explain import RuleQuality, RuleTable
    s = synthetic
    quads = np.array([[0, 0, 1, 0], [1, 1, 2, 1], [2, 0, 0, 1], [0, 2, 0, 0], [1, 2, 1, 0], [2, 2, 2, 0]], dtype=np.int32)
    tg = engine.TemporalGraph(3, 3, 2, quads)
    with pytest.raises(ValueError, match="rule_apply: temporal graph"):
        engine.rule_apply(tg, np.array([0]), np.array([[0, 1]]), np.array([0.5], np.float32), np.array([0]), np.array([0]))
    args = dict(head=s["head"], body=s["body"], weight=s["weight"], subs=s["subs"], rels=s["rels"])
    with pytest.raises(ValueError, match="rule_apply: head must be non-decreasing"):
        engine.rule_apply(s["graph"], **dict(args, head=s["head"][::-1].copy()))
    for bad in (0.0, 1.25, np.nan):
        w = s["weight"].copy()
        w[3] = bad
        with pytest.raises(ValueError, match=r"rule_apply: weights must be finite and in \(0, 1\]"):
            engine.rule_apply(s["graph"], **dict(args, weight=w))
    t = s["table"]
    quality = s["model"].rule_quality(t)
    wrong = RuleQuality(RuleTable(t.head, t.body, t.support, t.fixed, s["n_rel"] + 1), quality.body_pairs, quality.hits,
                        quality.pca_body_pairs, quality.head_pairs, quality.n_sources)
    with pytest.raises(ValueError, match="rule_scores: the table has n_rel=%d, the model n_rel=%d" % (s["n_rel"] + 1, s["n_rel"])):
        s["model"].rule_scores(wrong, s["subs"][:4], s["rels"][:4])
    with pytest.raises(ValueError, match="rule_scores: quality must be an explain.RuleQuality"):
        s["model"].rule_scores(t, s["subs"][:4], s["rels"][:4])
    with pytest.raises(ValueError, match="rule_predict: agg must be"):
        s["model"].rule_predict(quality, s["subs"][:4], s["rels"][:4], agg="mean")
    with pytest.raises(ValueError, match="rule_predict: k must be an integer in 1"):
        s["model"].rule_predict(quality, s["subs"][:4], s["rels"][:4], k=0)
    # the C entry point's own checks, before any launch
    dev = torch.device("cuda")
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)
    f32 = lambda n: torch.zeros(n, dtype=torch.float32, device=dev)
    slab = torch.tensor([0, 3], dtype=torch.int64, device=dev)
    scratch = torch.zeros(engine.rule_apply_scratch_bytes(3), dtype=torch.uint8, device=dev)
    out = (f32(3), f32(3), i32(3), i32(3))
    p = _lib.ptr

    def call(graph, n_rules=1, n_hops=2, n_words=3):
        _lib.check(_lib.lib().rg_rule_apply(graph, p(i32(1)), p(i32(2)), p(f32(1)), p(f32(1)), n_rules, n_hops, 0, p(i32(1)), p(i32(1)),
                                            p(i32(64)), 1, p(slab), n_words, p(scratch), 3, *(p(o) for o in out), _lib.stream_ptr()))
    with pytest.raises(_lib.NativeError, match="rg_rule_apply: NULL graph"):
        call(None)
    with pytest.raises(_lib.NativeError, match="rg_rule_apply: temporal graph"):
        call(tg.handle)
    for hops in (0, 33):
        with pytest.raises(_lib.NativeError, match="rg_rule_apply: n_hops=%d not in 1..32" % hops):
            call(s["graph"].handle, n_hops=hops)
    with pytest.raises(_lib.NativeError, match="rg_rule_apply: n_rules=65536 not in"):
        call(s["graph"].handle, n_rules=65536)
    with pytest.raises(_lib.NativeError, match="rg_rule_apply: n_words=0 is outside"):
        call(s["graph"].handle, n_words=0)
    assert not any(o.any() for o in out)


def test_relation_ids_are_bounded_in_the_kernel(synthetic):
    """The C entry point trusts its caller for the ids (engine.rule_apply validates them).  A rule whose head is -1 or 2^31 - 1 has no
    query and no slab; a rule whose body names such a relation reaches nothing; the one good rule between them gives what it gives
    alone.  Read in csrc/rule_apply.hip before this was run: rule_slab() tests the head against 0..n_rela_rows-1 before q_ptr is
    read, apply_hop_kernel tests the step's relation before rel_ptr is read, and the aggregate's search only meets heads >= 0."""
    from red_gnn_amd import _lib, engine
    s = synthetic
    g, dev, n_ent, n_rela = s["graph"], torch.device("cuda"), s["n_ent"], s["n_rela"]
    h = int(s["head"][0])
    mine = s["rels"] == h
    subs, B = s["subs"][mine], int(mine.sum())
    assert B > 0
    big = 2 ** 31 - 1
    good = s["body"][0].tolist()
    head = np.array([-1, h, h, h, big], np.int32)
    body = np.array([good, [good[0], -1, good[2]], good, [big, good[1], good[2]], good], np.int32)
    weight = np.array([0.5, 0.5, s["weight"][0], 0.5, 0.5], np.float32)
    q_ptr = np.zeros(n_rela + 1, np.int32)
    q_ptr[h + 1:] = B
    W = (B + 31) // 32
    slab = np.array([0, 0, 1, 2, 3, 3], np.int64) * n_ent * W                   # the rules of head h have a slab each
    to = lambda a: torch.from_numpy(a).to(dev)
    scratch = torch.empty(engine.rule_apply_scratch_bytes(int(slab[-1])), dtype=torch.uint8, device=dev)
    out = (torch.zeros((B, n_ent), dtype=torch.float32, device=dev), torch.ones((B, n_ent), dtype=torch.float32, device=dev),
           torch.full((B, n_ent), -1, dtype=torch.int32, device=dev), torch.zeros((B, n_ent), dtype=torch.int32, device=dev))
    p = _lib.ptr
    keep = [to(a) for a in (head, body, weight, A.miss_of(weight), subs.astype(np.int32), np.arange(B, dtype=np.int32), q_ptr, slab)]
    _lib.check(_lib.lib().rg_rule_apply(g.handle, p(keep[0]), p(keep[1]), p(keep[2]), p(keep[3]), 5, 3, 0, p(keep[4]), p(keep[5]),
                                        p(keep[6]), B, p(keep[7]), int(slab[-1]), p(scratch), 3, *(p(o) for o in out), _lib.stream_ptr()))
    ref = A.apply_dense(n_ent, n_rela, s["rows"], head[2:3], body[2:3], weight[2:3], subs, np.full(B, h), rule_base=2)
    assert A.same(_np(out), ref) and (ref[3] > 0).any()
