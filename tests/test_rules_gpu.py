"""top_paths on the digraphs model.explain returns, and the rule tables built from them (-m gpu): against strongest_paths, against
tests/paths_ref.py on the digraph copied to the host, and BaseModel.rules against the host reference batch by batch."""
import numpy as np
import pytest
import torch

from tests import _util as U
from tests import paths_ref as R

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


def _host_paths(rd, k):
    """(PathSet of the host reference on the digraph copied to the host, that copy)."""
    from red_gnn_amd.explain import PathSet, RDigraph
    host = RDigraph(rd.edges.cpu(), rd.alpha.cpu(), rd.offsets.cpu(), rd.reached.cpu(), rd.score.cpu(), rd.n_hops)
    edge, prod, count = R.dp(host.edges.numpy(), host.alpha.numpy(), host.offsets.numpy(), rd.n_hops, k)
    return PathSet(torch.from_numpy(edge), torch.from_numpy(prod), torch.from_numpy(count), host)


def _same_paths(ps, ref):
    return (torch.equal(ps.edge.cpu(), ref.edge) and torch.equal(ps.count.cpu(), ref.count)
            and ps.product.cpu().numpy().tobytes() == ref.product.numpy().tobytes())


def _same_table(a, b):
    a, b = a.cpu(), b.cpu()
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("head", "body", "support", "fixed")) and a.n_rel == b.n_rel


@pytest.fixture(scope="module")
def synthetic():
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(300, 7, 3000, seed=3)
    loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test),
                        verbose=False)
    torch.manual_seed(1234)
    model = RED_GNN_trans(P(3, 16, 5, loader.n_rel, "relu"), loader).cuda().eval()
    test = np.asarray(kg.test)[:24].astype(np.int64)
    return model, test[:, 0], test[:, 1], test[:, 2]


@pytest.mark.parametrize("min_alpha", [0.0, 0.2])
def test_top_paths_1_is_strongest_paths(synthetic, min_alpha):
    model, subs, rels, objs = synthetic
    for answers in (objs, None):                                             # the test tails (some unreached), the model's own answers
        rd = model.explain(subs, rels, answers, min_alpha=min_alpha)
        assert rd.edges.shape[0] > 0
        r, e, p = rd.strongest_paths()
        ps = rd.top_paths(1)
        assert torch.equal(ps.rels()[:, 0], r) and torch.equal(ps.entities()[:, 0], e)
        assert ps.product[:, 0].cpu().numpy().tobytes() == p.cpu().numpy().tobytes()
        assert torch.equal(ps.count.bool(), e[:, 0] >= 0)
        al = ps.alphas().double()[:, 0]                                        # the product again, from the gathered alphas
        got = (al[:, 0] * al[:, 1]) * al[:, 2]
        assert torch.equal(torch.where(ps.count > 0, got, torch.zeros_like(got)), ps.product[:, 0])


@pytest.mark.parametrize("min_alpha", [0.0, 0.2])
def test_top_paths_4_is_the_host_reference(synthetic, min_alpha):
    model, subs, rels, objs = synthetic
    rd = model.explain(subs, rels, objs, min_alpha=min_alpha)
    ref = _host_paths(rd, 4)
    assert int(ref.count.max()) == 4
    assert _same_paths(rd.top_paths(4), ref)
    table = model.rules(subs, rels, objs, k=4, min_alpha=min_alpha)
    from red_gnn_amd.explain import rules_from_paths
    assert _same_table(table, rules_from_paths(ref, rels, model.n_rel))
    assert int(table.support.sum()) == int(ref.count.sum())


def test_base_model_rules_family():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.explain import rules_from_paths, split_rows
    from red_gnn_amd.load_data import DataLoader
    loader = DataLoader(ids=U.load("family_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 64), loader)
    table = bm.rules("test", k=2, max_queries=100)
    subs, rels, objs, mode = split_rows(loader, "test", 100)
    assert mode == "test" and len(subs) >= 100 and len(subs) > 64              # more than one batch
    ref, n_paths = None, 0
    for lo in range(0, len(subs), 64):
        rd = bm.model.explain(subs[lo:lo + 64], rels[lo:lo + 64], objs[lo:lo + 64], mode=mode)
        paths = _host_paths(rd, 2)
        assert _same_paths(rd.top_paths(2), paths)
        n_paths += int(paths.count.sum())
        part = rules_from_paths(paths, rels[lo:lo + 64], loader.n_rel)
        ref = part if ref is None else ref + part
    assert _same_table(table, ref)
    assert int(table.support.sum()) == n_paths and n_paths > 0
    bm.n_tbatch = 17                                                          # the table does not depend on the batching
    assert _same_table(bm.rules("test", k=2, max_queries=100), table)
    assert len(table.format()) == table.head.numel() and table.top(int(table.head[0]), 3).head.numel() >= 1
    with pytest.raises(ValueError):
        bm.rules("train")
    with pytest.raises(ValueError):
        bm.rules("test", max_queries=0)


def test_base_model_rules_inductive():
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.explain import split_rows
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    loader = DataLoader(ids=U.load("ind_WN18RR_v1_ids.npz"), verbose=False)
    torch.manual_seed(7)
    bm = BaseModel(_opt(loader, 32), loader)
    assert isinstance(bm.model, RED_GNN_induc)
    table = bm.rules("test", k=2, max_queries=60)
    subs, rels, objs, mode = split_rows(loader, "test", 60)
    assert mode == loader.eval_mode("test")
    count = bm.model.explain(subs, rels, objs, mode=mode).top_paths(2).count
    assert int(table.support.sum()) == int(count.sum()) and int(count.sum()) > 0
    assert ((table.head >= 0) & (table.head < 2 * loader.n_rel)).all() and ((table.body >= 0) & (table.body <= 2 * loader.n_rel)).all()
