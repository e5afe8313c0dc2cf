"""Parity of the HIP path (through the C-ABI, libredgnn.so) against the oracle and the golden
fixtures generated from the reference.  Needs an MI355X: every test is marked ``gpu``.

Bars: node sets, old_nodes_new_idx, edge multisets and ranks bit-exact; fp32 values within
rtol 1e-4 of the reference's CPU results, with atol 1e-5 on scores and 5e-5 on hidden states
(O(1) values built from fp32 sums of up to ~300 terms per destination over up to 5 layers; the
reference's own sum order is unspecified, SURVEY.md §7 "Determinism / tolerance"), and
rtol 2e-3 / atol 2e-5 on gradients (sums over every edge of the batch).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import redgnn_oracle as orc
from tests import _util as U

pytestmark = pytest.mark.gpu

RTOL, ATOL, ATOL_H = 1e-4, 1e-5, 5e-5


class P:
    def __init__(self, n_layer, hidden_dim, attn_dim, n_rel, act, dropout=0.0):
        self.n_layer, self.hidden_dim, self.attn_dim, self.n_rel, self.act, self.dropout = n_layer, hidden_dim, attn_dim, n_rel, act, dropout


def make_model(fx, ids, train=False):
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    loader = DataLoader(ids=ids, verbose=False)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    model = RED_GNN_trans(P(n_layer, d, a, loader.n_rel, str(fx["act"])), loader).cuda()
    sd = {k: torch.tensor(v) for k, v in U.params_of(fx).items()}
    missing, unexpected = model.load_state_dict(sd, strict=True)
    model.train() if train else model.eval()
    return loader, model


def test_library_version_and_graph_export():
    from red_gnn_amd import _lib
    from red_gnn_amd.engine import Graph
    assert _lib.lib().rg_version() >= 1
    ids = U.load("tiny_fwd.npz")
    n_ent, n_rel = int(ids["n_ent"]), int(ids["n_rel"])
    base = np.concatenate([ids["facts"], ids["train"]], 0)
    g = Graph(n_ent, n_rel, base)
    og = orc.OracleGraph(orc.double_triple(base, n_rel), n_ent, n_rel)   # same fact-row order as rg_graph_create
    assert g.n_fact == og.n_fact == U.oracle_graph(ids, "test").n_fact
    op, ort, ip, ihr = g.export()
    assert np.array_equal(op, og.head_ptr)
    kg = og.KG[np.lexsort((np.arange(og.n_fact), og.KG[:, 1], og.KG[:, 0]))]   # grouped by head, then relation, then fact order
    assert np.array_equal(ort, kg[:, [1, 2]])
    order_t = np.argsort(og.KG[:, 2], kind="stable")
    assert np.array_equal(ihr, og.KG[order_t][:, [0, 1]])
    assert ip[-1] == og.n_fact


@pytest.mark.parametrize("name,ids", [("tiny_fwd.npz", None), ("family_d64.npz", "family_ids.npz"), ("umls_d48.npz", "umls_ids.npz")])
def test_get_neighbors_matches_oracle_every_hop(name, ids):
    """DataLoader.get_neighbors (HIP) vs the oracle's restatement of load_data.py:106-131, hop by hop."""
    from red_gnn_amd.load_data import DataLoader
    fx = U.load(name)
    ids = fx if ids is None else U.load(ids)
    loader = DataLoader(ids=ids, verbose=False)
    og = U.oracle_graph(ids, "test")
    nodes = np.stack([np.arange(len(fx["subs"])), fx["subs"]], 1).astype(np.int64)
    for i in range(int(fx["cfg"][0])):
        t_nodes, t_edges, t_old = orc.get_neighbors(og, nodes)
        g_nodes, g_edges, g_old = loader.get_neighbors(nodes, mode="test")
        assert g_nodes.dtype == torch.int64 and g_nodes.is_cuda
        assert np.array_equal(g_nodes.cpu().numpy(), t_nodes)
        assert np.array_equal(g_nodes.cpu().numpy(), fx["L%d_nodes" % i])
        assert np.array_equal(g_old.cpu().numpy(), t_old)
        ge = g_edges.cpu().numpy()
        assert ge.shape == t_edges.shape
        assert np.array_equal(U.sorted_edges(ge), U.sorted_edges(t_edges))     # all six columns, as a multiset
        assert U.edge_multiset_hash(ge) == str(fx["L%d_edge_hash" % i])
        assert np.all(np.diff(ge[:, 5]) >= 0)                                   # destination-segmented
        nodes = t_nodes


@pytest.mark.parametrize("name,ids", [("tiny_fwd.npz", None), ("family_d48.npz", "family_ids.npz"),
                                      ("family_d64.npz", "family_ids.npz"), ("umls_d48.npz", "umls_ids.npz")])
def test_forward_matches_reference_fixture(name, ids):
    fx = U.load(name)
    ids = fx if ids is None else U.load(ids)
    loader, model = make_model(fx, ids)
    trace = []
    with torch.no_grad():
        scores = model(fx["subs"], fx["rels"], mode=str(fx["mode"]), trace=trace)
    assert scores.is_cuda and scores.dtype == torch.float32 and tuple(scores.shape) == fx["scores"].shape
    for i, t in enumerate(trace):
        assert np.array_equal(t["nodes"].cpu().numpy(), fx["L%d_nodes" % i])
        assert np.array_equal(t["old_nodes_new_idx"].cpu().numpy(), fx["L%d_old_nodes_new_idx" % i])
        assert t["n_edges"] == int(fx["L%d_n_edges" % i])
        if "L%d_hidden" % i in fx:
            np.testing.assert_allclose(t["hidden"].cpu().numpy(), fx["L%d_hidden" % i], rtol=RTOL, atol=ATOL_H)
    s = scores.cpu().numpy()
    np.testing.assert_allclose(s, fx["scores"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(s == 0, fx["scores"] == 0)          # exact zeros at unvisited entities
    # filtered ranks of this batch, on the device
    from red_gnn_amd.utils import cal_ranks
    n_ent = loader.n_ent
    if "labels" in fx:
        labels, filt = fx["labels"], fx["filters"]
    else:
        labels = np.zeros((len(fx["subs"]), n_ent)); labels[fx["labels_idx"][:, 0], fx["labels_idx"][:, 1]] = 1
        filt = np.zeros((len(fx["subs"]), n_ent)); filt[fx["filters_idx"][:, 0], fx["filters_idx"][:, 1]] = 1
    assert np.array_equal(np.array(cal_ranks(fx["scores"], labels, filt)), fx["ranks"])
    # ... and the composition forward -> rank kernel on the GPU's own scores: equal to the oracle's ranking of those scores,
    # and equal to the reference's ranks except where two scores sit within rounding of each other
    gpu_ranks = np.array(cal_ranks(s, labels, filt))
    assert np.array_equal(gpu_ranks, np.array(orc.cal_ranks(s, labels, filt)))
    assert np.mean(gpu_ranks != fx["ranks"]) <= 0.02, (gpu_ranks, fx["ranks"])


def test_forward_wn18rr_node_sets():
    fx, ids = U.load("WN18RR_d48.npz"), U.load("WN18RR_ids.npz")
    loader, model = make_model(fx, ids)
    trace = []
    with torch.no_grad():
        scores = model(fx["subs"], fx["rels"], mode="test", trace=trace)
    for i, t in enumerate(trace):
        nodes = t["nodes"].cpu().numpy()
        assert len(nodes) == int(fx["L%d_n_nodes" % i])
        assert U.sha(nodes.astype(np.int64)) == str(fx["L%d_nodes_hash" % i])
        assert t["n_edges"] == int(fx["L%d_n_edges" % i])
    vis = trace[-1]["nodes"].cpu().numpy()
    s = scores.cpu().numpy()
    np.testing.assert_allclose(s[vis[:, 0], vis[:, 1]], fx["scores_visited"], rtol=RTOL, atol=ATOL_H)   # 5 layers deep
    assert np.count_nonzero(s) == int(fx["score_nnz"])


def test_backward_matches_reference_fixture():
    fx = U.load("tiny_bwd.npz")
    loader, model = make_model(fx, fx, train=True)
    scores = model(fx["subs"], fx["rels"], mode="train")
    from red_gnn_amd.base_model import reference_loss
    loss = reference_loss(scores, torch.as_tensor(fx["tails"], dtype=torch.long, device=scores.device))
    assert abs(loss.item() - float(fx["loss"])) < 1e-4 * abs(float(fx["loss"]))
    loss.backward()
    grads = U.grads_of(fx)
    for k, p in model.named_parameters():
        np.testing.assert_allclose(p.grad.cpu().numpy(), grads[k], rtol=2e-3, atol=1e-5, err_msg=k)


def test_rank_kernel_heavy_ties():
    from red_gnn_amd.utils import cal_ranks, cal_performance
    fx = U.load("ranks.npz")
    ranks = cal_ranks(fx["scores"], fx["labels"], fx["filters"])
    assert np.array_equal(np.array(ranks), fx["ranks"])
    np.testing.assert_allclose(np.array(cal_performance(ranks)), fx["perf"], rtol=1e-12)


def _random_model(loader, n_layer, d, a, act, seed=1234):
    from red_gnn_amd.models import RED_GNN_trans
    torch.manual_seed(seed)
    model = RED_GNN_trans(P(n_layer, d, a, loader.n_rel, act), loader).cuda().eval()
    return model


@pytest.mark.parametrize("d,a,act,n_layer", [(16, 3, "idd", 2), (20, 5, "tanh", 3), (32, 5, "relu", 3), (48, 5, "relu", 3),
                                            (64, 5, "relu", 3), (128, 10, "relu", 2), (30, 30, "tanh", 2), (256, 5, "relu", 2), (100, 12, "tanh", 2),
                                            (48, 20, "relu", 2), (64, 27, "tanh", 2), (32, 17, "idd", 2)])
def test_forward_vs_oracle_dims(d, a, act, n_layer):
    """Every hidden/attention width the reference's presets use, incl. d % 4 != 0."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(300, 7, 3000, seed=3)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, n_layer, d, a, act)
    rng = np.random.default_rng(0)
    subs, rels = rng.integers(0, kg.n_ent, 9), rng.integers(0, 2 * kg.n_rel, 9)
    with torch.no_grad():
        s = model(subs, rels, mode="test").cpu().numpy()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = orc.forward(p, U.oracle_graph(ids, "test"), subs, rels, n_layer, act=act).numpy()
    np.testing.assert_allclose(s, ref, rtol=RTOL, atol=ATOL)
    assert np.array_equal(s == 0, ref == 0)


def test_forward_vs_oracle_c2_shape_small_batch():
    """BASELINE config 2 (10k entities / 50 relations / 200k triples, L=3, d=64) at a batch the oracle
    finishes in seconds; hubs with in-degree in the thousands exercise the long-row path."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_shape
    kg = make_shape("C2")
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, 64, 5, "relu")
    subs, rels = kg.test[:6, 0], kg.test[:6, 1]
    trace = []
    with torch.no_grad():
        s = model(subs, rels, mode="test", trace=trace).cpu().numpy()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    otrace = []
    ref = orc.forward(p, U.oracle_graph(ids, "test"), subs, rels, 3, act="relu", trace=otrace).numpy()
    for t, o in zip(trace, otrace):
        assert np.array_equal(t["nodes"].cpu().numpy(), o["nodes"])
        assert t["n_edges"] == len(o["edges"])
    np.testing.assert_allclose(s, ref, rtol=RTOL, atol=2e-5)


@pytest.mark.parametrize("B", [3, 6, 40, 400])
def test_level_build_paths_give_the_reference_node_lists(B):
    """The ways a new level's node list is built - one workgroup with its node list fused (B x ceil(n_ent / 32) <= 1 024 words) or as
    a launch of its own (<= 12 288 words), the general multi-launch transpose + scan + pack - against a dense numpy expansion on C2
    (313 words per query: 3 queries = 939 words, 6 = 1 878; 40 = 12 520 and 400 are the general path): node lists in (query, entity)
    order, links to the previous level, and the edge count of every hop.  expand() + nodes() pass no node buffer into the level build:
    the fused and the split node emission are tests/test_frontier_gpu.py's."""
    from red_gnn_amd import engine
    _, kg, ids, loader = _shape_loader("C2")
    g = loader.graph_for("test")
    rng = np.random.default_rng(B)
    heads = rng.integers(0, kg.n_ent, B).astype(np.int32)
    trip = np.concatenate([kg.facts, kg.train], 0)
    src = np.concatenate([trip[:, 0], trip[:, 2], np.arange(kg.n_ent)])      # facts, inverses, self loops
    dst = np.concatenate([trip[:, 2], trip[:, 0], np.arange(kg.n_ent)])
    outdeg = np.bincount(src, minlength=kg.n_ent)
    adj = np.zeros((kg.n_ent, kg.n_ent), dtype=bool)
    adj[src, dst] = True
    fr = engine.Frontier(kg.n_ent, B, 2, "cuda")
    fr.reset(torch.as_tensor(heads, device="cuda"))
    cur = np.zeros((B, kg.n_ent), dtype=bool)
    cur[np.arange(B), heads] = True
    for hop in range(3):
        n_new, n_e, n_old = fr.expand(g)
        nodes, prev_idx, _ = fr.nodes(want_prev=True, want_old_new=False)
        nxt = (cur.astype(np.float32) @ adj.astype(np.float32)) > 0
        want = np.argwhere(nxt)
        assert n_new == len(want) and n_old == int(cur.sum())
        assert n_e == int((cur * outdeg[None, :]).sum())
        assert np.array_equal(nodes.cpu().numpy(), want)
        old = np.argwhere(cur)
        rank_old = -np.ones((B, kg.n_ent), dtype=np.int64)
        rank_old[old[:, 0], old[:, 1]] = np.arange(len(old))
        assert np.array_equal(prev_idx.cpu().numpy(), rank_old[want[:, 0], want[:, 1]])
        cur = nxt


def _shape_loader(cfg):
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import SHAPES, make_shape
    kg = make_shape(cfg)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    return SHAPES[cfg], kg, ids, DataLoader(ids=ids, verbose=False)


@pytest.mark.parametrize("cfg,B", [("C3", 3), ("C4", 2)])
def test_forward_vs_oracle_baseline_shapes_c3_c4(cfg, B):
    """BASELINE configs[2] (WN18RR-shaped: 40k entities / 11 relations / 93k triples, 5 hops, d=64) and configs[3]
    (FB15k-237-shaped: 15k / 237 / 310k, 4 hops, d=128: 475-row relation table, streamed-weights dense kernel) at their
    named sizes, at a batch the oracle finishes in seconds: node sets bit-exact every hop, scores within tolerance, and the
    filtered ranks of the GPU's scores equal to the oracle's ranking."""
    from red_gnn_amd.utils import cal_ranks_csr
    sh, kg, ids, loader = _shape_loader(cfg)
    L, d, a = sh["n_layer"], sh["hidden_dim"], sh["attn_dim"]
    model = _random_model(loader, L, d, a, "relu")
    subs, rels, ap, ai, fp, fi = loader.get_batch_csr(np.arange(B), data="test")
    trace, otrace = [], []
    with torch.no_grad():
        scores = model(subs, rels, mode="test", trace=trace)
        ranks = cal_ranks_csr(scores, ap, ai, fp, fi).double().cpu().numpy()
    s = scores.cpu().numpy()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    og = U.oracle_graph(ids, "test")
    ref = orc.forward(p, og, subs, rels, L, act="relu", trace=otrace).numpy()
    o64 = []
    ref64 = orc.forward(p, og, subs, rels, L, act="relu", dtype=torch.float64, trace=o64).numpy()
    assert len(trace) == len(otrace) == L
    for i, (t, o, o6) in enumerate(zip(trace, otrace, o64)):
        assert np.array_equal(t["nodes"].cpu().numpy(), o["nodes"])
        assert np.array_equal(t["old_nodes_new_idx"].cpu().numpy(), o["old_nodes_new_idx"])
        assert t["n_edges"] == len(o["edges"])
        # up to 5 hops deep, sums of thousands of fp32 terms at hub destinations: see _util.assert_close_fp32
        U.assert_close_fp32(t["hidden"].cpu().numpy(), o["hidden"].numpy(), o6["hidden"].numpy(), RTOL, ATOL_H, "hidden of hop %d" % i)
    U.assert_close_fp32(s, ref, ref64, RTOL, ATOL_H, "scores")
    assert np.array_equal(s == 0, ref == 0)
    labels, filt = np.zeros((B, kg.n_ent)), np.zeros((B, kg.n_ent))
    api, aii, fpi, fii = (t.cpu().numpy() for t in (ap, ai, fp, fi))
    for q in range(B):
        labels[q, aii[api[q]:api[q + 1]]] = 1
        filt[q, fii[fpi[q]:fpi[q + 1]]] = 1
    assert np.array_equal(ranks, np.array(orc.cal_ranks(s, labels, filt)))


@pytest.mark.parametrize("cfg", ["C3", "C4"])
def test_full_size_properties_c3_c4(cfg):
    """The same shapes at a bench batch (B=64), through properties that need no oracle run: two runs bit-identical; a
    query's row does not depend on its batch mates (permutation, sub-batch); frontiers sorted, unique and monotone;
    E of every hop = sum of the out-degrees of the previous frontier."""
    sh, kg, ids, loader = _shape_loader(cfg)
    model = _random_model(loader, sh["n_layer"], sh["hidden_dim"], sh["attn_dim"], "relu")
    B = 64
    subs, rels = kg.test[:B, 0], kg.test[:B, 1]
    perm = np.random.default_rng(1).permutation(B)
    trace = []
    with torch.no_grad():
        s1 = model(subs, rels, mode="test", trace=trace)
        s2 = model(subs, rels, mode="test")
        sp = model(subs[perm], rels[perm], mode="test")
        ss = model(subs[40:47], rels[40:47], mode="test")
    assert torch.equal(s1, s2)
    for got, want in ((sp, s1[perm]), (ss, s1[40:47])):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
        assert torch.equal(got == 0, want == 0)
    outdeg = np.diff(U.oracle_graph(ids, "test").head_ptr)
    prev = np.stack([np.arange(B), subs], 1)
    for t in trace:
        nodes = t["nodes"].cpu().numpy()
        key = nodes[:, 0].astype(np.int64) * kg.n_ent + nodes[:, 1]
        assert np.all(np.diff(key) > 0)
        assert np.all(np.isin(prev[:, 0].astype(np.int64) * kg.n_ent + prev[:, 1], key))
        assert t["n_edges"] == int(outdeg[prev[:, 1]].sum())
        prev = nodes


def _c5_model(seed=7):
    from red_gnn_amd.synthetic import SHAPES, make_temporal_shape
    sh, tkg = SHAPES["C5"], make_temporal_shape("C5")
    fx = dict(quads=tkg.quads, n_ent=tkg.n_ent, n_rel=tkg.n_rel, n_time=tkg.n_time)
    # tanh: five hops of unnormalised relu sums reach 1e7 with random weights, where fp32 cancellation is all one would measure
    return sh, tkg, fx, _temporal_model(fx, False, sh["n_layer"], sh["hidden_dim"], sh["attn_dim"], "tanh", seed=seed)


def test_temporal_c5_shape_vs_oracle():
    """BASELINE configs[4] at its named size (7k entities / 230 relations + inverses + idd = 461 relation rows / 365
    timestamps + sentinel / 90k quadruples -> 187k graph rows, 5 hops, d=64, attention width 30; per-layer tables as
    model_cuda.py) at a batch the oracle finishes in seconds.  Parity of this layout is pinned through model.py's fixture
    for the shared arithmetic only (see test_temporal_matches_reference_model_py_fixture): unpinned for what differs."""
    sh, tkg, fx, model = _c5_model()
    B = 3
    q = tkg.quads[:B]
    batch = {"head": q[:, 0], "relation": q[:, 1], "time": q[:, 3]}
    with torch.no_grad():
        s = model(batch, mode="test").cpu().numpy()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    otrace = []
    ref = orc.temporal_forward(p, tkg.quads, tkg.n_ent, batch["head"], batch["relation"], batch["time"], sh["n_layer"], "tanh",
                               trace=otrace).numpy()
    ref64 = orc.temporal_forward(p, tkg.quads, tkg.n_ent, batch["head"], batch["relation"], batch["time"], sh["n_layer"], "tanh",
                                 dtype=torch.float64).numpy()
    assert model.last_stats["n_edges"] == [t["n_edges"] for t in otrace]
    assert np.array_equal(model.last_nodes.cpu().numpy(), otrace[-1]["nodes"])
    U.assert_close_fp32(s, ref, ref64, RTOL, ATOL_H, "scores")
    assert np.array_equal(s == 0, ref == 0)


def test_temporal_c5_full_size_properties():
    """C5 at B=64: determinism, permutation and sub-batch invariance of every query's row."""
    sh, tkg, fx, model = _c5_model()
    B = 64
    q = tkg.quads[:B]
    perm = np.random.default_rng(2).permutation(B)
    mk = lambda rows: {"head": rows[:, 0], "relation": rows[:, 1], "time": rows[:, 3]}
    with torch.no_grad():
        s1 = model(mk(q), mode="test")
        s2 = model(mk(q), mode="test")
        sp = model(mk(q[perm]), mode="test")
        ss = model(mk(q[10:15]), mode="test")
    assert torch.equal(s1, s2)
    for got, want in ((sp, s1[perm]), (ss, s1[10:15])):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
        assert torch.equal(got == 0, want == 0)


def test_backward_vs_oracle_autograd():
    """Gradients of every parameter on a KG larger than the tiny fixture (LDS-privatised relation
    gradients, multi-block flush), against torch autograd through the oracle."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    from red_gnn_amd.base_model import reference_loss
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(400, 6, 4000, seed=11)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    torch.manual_seed(5)
    model = RED_GNN_trans(P(3, 32, 5, loader.n_rel, "tanh"), loader).cuda().train()
    trip = loader.train_data[:12]
    scores = model(trip[:, 0], trip[:, 1], mode="train")
    loss = reference_loss(scores, torch.as_tensor(trip[:, 2], device=scores.device))
    loss.backward()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    os_ = orc.forward(p, U.oracle_graph(ids, "train"), trip[:, 0], trip[:, 1], 3, act="tanh")
    ol = orc.loss_fn(os_, trip[:, 2])
    ol.backward()
    assert abs(loss.item() - ol.item()) < 1e-4 * abs(ol.item())
    for k, v in model.named_parameters():
        np.testing.assert_allclose(v.grad.cpu().numpy(), p[k].grad.numpy(), rtol=2e-3, atol=2e-5, err_msg=k)


@pytest.mark.parametrize("a", [5, 20])
def test_two_forwards_before_backward(a):
    """Two grad-enabled forwards of the same batch size before the first backward (gradient accumulation, two losses): each
    autograd graph keeps its own frontier (engine.FrontierLease), the accumulated gradients equal autograd through the oracle.
    a = 20: an attention width between the kernels' instantiated paddings (17..28 -> 32)."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(350, 6, 3500, seed=13)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, 32, a, "tanh", seed=4).train()
    rng = np.random.default_rng(8)
    B = 11
    qa, qb = (np.stack([rng.integers(0, kg.n_ent, B), rng.integers(0, 2 * kg.n_rel, B)], 1) for _ in range(2))
    wa, wb = (torch.tensor(rng.standard_normal((B, kg.n_ent)), dtype=torch.float32) for _ in range(2))
    s_a = model(qa[:, 0], qa[:, 1], mode="train")
    s_b = model(qb[:, 0], qb[:, 1], mode="train")                     # same shape: must not reuse s_a's frontier
    with torch.no_grad():
        model.eval()
        model(qa[:, 0], qa[:, 1], mode="train")                       # an inference forward in between (own frontier as well)
        model.train()
    (s_a * wa.cuda()).sum().backward()
    (s_b * wb.cuda()).sum().backward()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    og = U.oracle_graph(ids, "train")
    r_a = orc.forward(p, og, qa[:, 0], qa[:, 1], 3, act="tanh")
    r_b = orc.forward(p, og, qb[:, 0], qb[:, 1], 3, act="tanh")
    np.testing.assert_allclose(s_a.detach().cpu().numpy(), r_a.detach().numpy(), rtol=RTOL, atol=ATOL_H)
    np.testing.assert_allclose(s_b.detach().cpu().numpy(), r_b.detach().numpy(), rtol=RTOL, atol=ATOL_H)
    ((r_a * wa).sum() + (r_b * wb).sum()).backward()
    for k, v in model.named_parameters():
        r = p[k].grad.numpy()
        np.testing.assert_allclose(v.grad.cpu().numpy(), r, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(r).max())), err_msg=k)
    # and the guard itself: a reset behind a live lease is reported, not silently wrong
    from red_gnn_amd import engine
    s_c = model(qa[:, 0], qa[:, 1], mode="train")
    leased = [f for frs in model._frontiers.pool.values() for f in frs if f.leases > 0]
    assert len(leased) == 1
    leased[0].reset(torch.as_tensor(qb[:, 0], dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="reset by a later forward"):
        s_c.sum().backward()


@pytest.mark.parametrize("d,a,B,n_ent,m", [(16, 3, 1, 40, 300), (20, 5, 31, 150, 2500), (64, 5, 33, 300, 6000), (48, 12, 70, 90, 4000),
                                           (128, 5, 9, 200, 3000), (256, 20, 5, 120, 1500)])
def test_word_parallel_walk_bitwise_equals_per_query_walk(d, a, B, n_ent, m):
    """rg_layer_fwd's two edge walks (per destination / word-parallel from the frontier's nodes, 32, 16, 8, 4, 2 or 1 queries per item)
    enumerate the same edges and sum them in the same order: every hop's hidden state and the scores are bitwise equal, on
    sparse and saturated hops alike, with hub rows cut into segments (in-degree > 128), lane groups of 4..64, batch sizes
    around the 32-query word, isolated entities, and an automatic pick that matches one of them."""
    from red_gnn_amd import engine
    from red_gnn_amd.load_data import DataLoader
    rng = np.random.default_rng(d * 1000 + B)
    n_rel = 4
    h, t = rng.integers(0, n_ent - 3, m), rng.integers(0, n_ent - 3, m)            # the last entities stay isolated
    t[: m // 3] = int(rng.integers(0, n_ent - 3))                                   # a hub destination: several segments
    facts = np.stack([h, rng.integers(0, n_rel, m), t], 1)
    ids = _ids(n_ent, n_rel, facts[: (3 * m) // 4], train=facts[(3 * m) // 4:])
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, d, a, "tanh", seed=B)
    model.use_graphs = False
    subs, rels = rng.integers(0, n_ent, B), rng.integers(0, 2 * n_rel, B)
    subs[-1] = n_ent - 1
    outs = {}
    try:
        with torch.no_grad():
            for walk in (1, 2, 3, 4, 5, 6, 7, 0):
                engine.FORCE_WALK = walk
                trace = []
                s = model(subs, rels, mode="test", trace=trace)
                outs[walk] = (s, [x["hidden"].clone() for x in trace])
    finally:
        engine.FORCE_WALK = 0
    for walk in (2, 3, 4, 5, 6, 7, 0):
        assert torch.equal(outs[walk][0], outs[1][0]), walk
        for x, y in zip(outs[walk][1], outs[1][1]):
            assert torch.equal(x, y), walk
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = orc.forward(p, U.oracle_graph(ids, "test"), subs, rels, 3, act="tanh").numpy()
    np.testing.assert_allclose(outs[2][0].cpu().numpy(), ref, rtol=RTOL, atol=ATOL_H)


def test_word_parallel_walk_in_training_matches_oracle_gradients():
    """The training forward (autograd path, rg_layer_fwd + rg_layer_bwd) with the word-parallel walk forced on every hop."""
    from red_gnn_amd import engine
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(250, 5, 2500, seed=19)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, 32, 5, "relu", seed=2).train()
    rng = np.random.default_rng(4)
    B = 13
    subs, rels = rng.integers(0, kg.n_ent, B), rng.integers(0, 2 * kg.n_rel, B)
    w = torch.tensor(rng.standard_normal((B, kg.n_ent)), dtype=torch.float32)
    try:
        engine.FORCE_WALK = 2
        s = model(subs, rels, mode="train")
    finally:
        engine.FORCE_WALK = 0
    (s * w.cuda()).sum().backward()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    ref = orc.forward(p, U.oracle_graph(ids, "train"), subs, rels, 3, act="relu")
    np.testing.assert_allclose(s.detach().cpu().numpy(), ref.detach().numpy(), rtol=RTOL, atol=ATOL_H)
    (ref * w).sum().backward()
    for k, v in model.named_parameters():
        r = p[k].grad.numpy()
        np.testing.assert_allclose(v.grad.cpu().numpy(), r, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(r).max())), err_msg=k)


def test_full_size_properties_c2():
    """BASELINE config 2 at bench batch size: properties that need no oracle run.
    (1) per-query independence: a query's score row does not depend on its batch mates;
    (2) determinism: two runs are bit-identical (destination-ordered sums, no float atomics);
    (3) visited sets grow monotonically and edge counts equal sum of out-degrees of the frontier."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_shape
    kg = make_shape("C2")
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, 64, 5, "relu")
    B = 256
    subs, rels = kg.test[:B, 0], kg.test[:B, 1]
    trace = []
    with torch.no_grad():
        s1 = model(subs, rels, mode="test", trace=trace)
        s2 = model(subs, rels, mode="test")
        s_sub = model(subs[100:108], rels[100:108], mode="test")
    assert torch.equal(s1, s2)
    # (the dense GEMMs are rocBLAS calls whose tiling depends on the row count, so not bitwise)
    np.testing.assert_allclose(s_sub.cpu().numpy(), s1[100:108].cpu().numpy(), rtol=RTOL, atol=ATOL)
    assert torch.equal(s_sub == 0, s1[100:108] == 0)
    og = U.oracle_graph(ids, "test")
    outdeg = np.diff(og.head_ptr)
    prev = np.stack([np.arange(B), subs], 1)
    for t in trace:
        nodes = t["nodes"].cpu().numpy()
        key = nodes[:, 0].astype(np.int64) * kg.n_ent + nodes[:, 1]
        assert np.all(np.diff(key) > 0)                                  # sorted, unique
        pkey = prev[:, 0].astype(np.int64) * kg.n_ent + prev[:, 1]
        assert np.all(np.isin(pkey, key))                                # monotone frontier
        assert t["n_edges"] == int(outdeg[prev[:, 1]].sum())             # E = sum of out-degrees
        prev = nodes


@pytest.mark.parametrize("prec", ["f32", "f16x2", "f16x3"])
@pytest.mark.parametrize("d,a,act", [(64, 5, "relu"), (48, 5, "tanh"), (32, 3, "idd"), (20, 10, "relu"), (30, 16, "tanh"), (128, 5, "relu")])
def test_fused_dense_kernel_matches_torch_dense_path(d, a, act, prec):
    """rg_dense_fwd (W_h + act + GRU + next a_s + readout on the matrix cores, as exact fp32 MFMA and as two-term f16 splits)
    against the same model with the dense part in torch ops (rocBLAS + gru_cell): same nodes, hidden and scores."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(700, 9, 9000, seed=21)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, d, a, act, seed=7)
    model.dense_precision = prec
    rng = np.random.default_rng(1)
    subs, rels = rng.integers(0, kg.n_ent, 37), rng.integers(0, 2 * kg.n_rel, 37)
    t1, t2 = [], []
    with torch.no_grad():
        model.fused_dense = True
        s1 = model(subs, rels, mode="test", trace=t1)
        model.fused_dense = False
        s2 = model(subs, rels, mode="test", trace=t2)
    for x, y in zip(t1, t2):
        assert torch.equal(x["nodes"], y["nodes"])
        np.testing.assert_allclose(x["hidden"].cpu().numpy(), y["hidden"].cpu().numpy(), rtol=RTOL, atol=ATOL_H)
    np.testing.assert_allclose(s1.cpu().numpy(), s2.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
    assert torch.equal(s1 == 0, s2 == 0)


def test_training_learns_on_family():
    """End-to-end drop-in check on real data: the reference's loop (BaseModel.train_batch: forward, the
    reference's loss, HIP backward, Adam, NaN scrub, filtered evaluation on the device) learns family.
    The reference reaches MRR ~0.98 after tens of epochs; here a fraction of one epoch must already lift the
    validation MRR far above the untrained model's."""
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.utils import cal_performance
    ids = U.load("family_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class Opt:
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch, n_tbatch = \
            0.0036, 0.999, 0.000017, 48, 5, 3, 0.29, "relu", 20, 50
        n_rel = loader.n_rel

    np.random.seed(1234)
    torch.manual_seed(1234)
    bm = BaseModel(Opt, loader)
    bm.model.eval()
    mrr0, _, _ = bm._performance(bm._rank_split("valid", 500))
    bm.n_valid, bm.n_test = 500, 200            # keep the test short: evaluate on a slice
    mrr1, out = bm.train_batch(epoch=0, max_batches=150)
    assert np.isfinite(bm.last_epoch_loss)
    assert mrr1 > max(0.5, 3 * mrr0), (mrr0, mrr1, out)


@pytest.mark.parametrize("mode", ["transductive", "inductive"])
def test_inductive_setting_matches_reference_fixture(mode):
    """Static/inductive: two-graph loader, RED_GNN_induc; n_ent switches with the mode."""
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    from red_gnn_amd.utils import cal_ranks
    fx, ids = U.load("ind_WN18RR_v1_%s.npz" % mode), U.load("ind_WN18RR_v1_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)
    n_layer, d, a = (int(x) for x in fx["cfg"])
    model = RED_GNN_induc(P(n_layer, d, a, loader.n_rel, str(fx["act"])), loader).cuda().eval()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    trace = []
    with torch.no_grad():
        scores = model(fx["subs"], fx["rels"], mode=mode, trace=trace)
    for i, t in enumerate(trace):
        assert np.array_equal(t["nodes"].cpu().numpy(), fx["L%d_nodes" % i])
        assert np.array_equal(t["old_nodes_new_idx"].cpu().numpy(), fx["L%d_old_nodes_new_idx" % i])
        assert t["n_edges"] == int(fx["L%d_n_edges" % i])
        np.testing.assert_allclose(t["hidden"].cpu().numpy(), fx["L%d_hidden" % i], rtol=RTOL, atol=ATOL_H)
    n_ent = loader.n_ent if mode == "transductive" else loader.n_ent_ind
    assert tuple(scores.shape) == (len(fx["subs"]), n_ent) == fx["scores"].shape
    np.testing.assert_allclose(scores.cpu().numpy(), fx["scores"], rtol=RTOL, atol=ATOL)
    labels = np.zeros(fx["scores"].shape); labels[fx["labels_idx"][:, 0], fx["labels_idx"][:, 1]] = 1
    filt = np.zeros(fx["scores"].shape); filt[fx["filters_idx"][:, 0], fx["filters_idx"][:, 1]] = 1
    assert np.array_equal(np.array(cal_ranks(fx["scores"], labels, filt)), fx["ranks"])
    # loader parity: queries and filters as the reference built them
    data = "valid" if mode == "transductive" else "test"
    subs, rels, ap, ai, fp, fi = loader.get_batch_csr(np.arange(len(fx["subs"])), data=data)
    assert np.array_equal(subs, fx["subs"]) and np.array_equal(rels, fx["rels"])
    assert np.array_equal(ai.cpu().numpy(), fx["labels_idx"][:, 1]) and np.array_equal(fi.cpu().numpy(), fx["filters_idx"][:, 1])


class TP:
    pass


def _temporal_model(fx, shared, n_layer, d, a, act, seed=None):
    from red_gnn_amd.temporal import T_RED_GNN
    p = TP()
    p.n_rel, p.n_ent, p.n_time = int(fx["n_rel"]), int(fx["n_ent"]), int(fx["n_time"])
    p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.graph, p.device = d, a, n_layer, act, fx["quads"], "cuda"
    if seed is not None:
        torch.manual_seed(seed)
    return T_RED_GNN(p, shared_tables=shared).cuda().eval()


def test_temporal_matches_reference_model_py_fixture():
    """T-RED-GNN interpolation forward (rg_tlayer_fwd) vs the output of the reference's model.py."""
    fx = U.load("temporal_model_py.npz")
    n_layer, d, a = (int(x) for x in fx["cfg"])
    model = _temporal_model(fx, True, n_layer, d, a, str(fx["act"]))
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    s = model({"head": fx["heads"], "relation": fx["rels"], "time": fx["times"]}, mode="test").detach().cpu().numpy()
    np.testing.assert_allclose(s, fx["scores"], rtol=RTOL, atol=ATOL)
    assert np.array_equal(s == 0, fx["scores"] == 0)


@pytest.mark.parametrize("d,a,act,n_layer", [(64, 30, "relu", 3), (32, 5, "tanh", 4), (20, 30, "idd", 2)])
def test_temporal_per_layer_tables_vs_oracle(d, a, act, n_layer):
    """model_cuda.py's layout (per-layer relation / attention tables) on an ICEWS14-shaped synthetic graph with hubs,
    against the oracle (this variant cannot be imported in the build container: parity pinned through model.py only)."""
    rng = np.random.default_rng(3)
    n_ent, n_rel, n_time, n_q = 400, 12, 365, 6000
    w = 1.0 / np.arange(1, n_ent + 1); w /= w.sum()
    h, t = rng.choice(n_ent, n_q, p=w), rng.integers(0, n_ent, n_q)
    quads = np.stack([h, rng.integers(0, n_rel - 1, n_q), t, rng.integers(0, n_time - 1, n_q)], 1)
    quads = np.concatenate([quads, quads[:, [2, 1, 0, 3]]], 0)                      # inverse direction keeps hubs as tails too
    idd = np.stack([np.arange(n_ent), np.full(n_ent, n_rel - 1), np.arange(n_ent), np.full(n_ent, n_time - 1)], 1)
    fx = dict(quads=np.concatenate([quads, idd], 0).astype(np.int32), n_ent=n_ent, n_rel=n_rel, n_time=n_time)
    model = _temporal_model(fx, False, n_layer, d, a, act, seed=9)
    B = 7
    batch = {"head": quads[:B, 0], "relation": quads[:B, 1], "time": quads[:B, 3]}
    with torch.no_grad():
        s = model(batch, mode="test").cpu().numpy()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = orc.temporal_forward(p, fx["quads"], n_ent, batch["head"], batch["relation"], batch["time"], n_layer, act).numpy()
    np.testing.assert_allclose(s, ref, rtol=RTOL, atol=ATOL_H)
    assert np.array_equal(s == 0, ref == 0)


@pytest.mark.parametrize("d,a,act,n_layer,B", [(32, 5, "tanh", 3, 9), (64, 30, "relu", 2, 40), (20, 3, "idd", 2, 3)])
def test_temporal_extrapolation_vs_oracle(d, a, act, n_layer, B):
    """T-RED-GNN extrapolation (per-query 120-step time windows over ONE device graph, self-loops, past_linear only,
    periodic time embedding, per-query softmax over the visited entities) against the oracle's restatement of
    model_cuda_new_embedding.py:135-261 - parity UNPINNED (that file cannot be imported here).  The data have days without rows
    (offset quirk of utils.py:692-699), queries older and younger than the window length, hub objects and duplicate rows."""
    from red_gnn_amd import extrapolation as X
    rng = np.random.default_rng(d + B)
    n_ent, n_rel, n = 120, 6, 5000
    days = np.sort(rng.choice(np.delete(np.arange(200), [0, 50, 51, 120]), n))
    w = 1.0 / np.arange(1, n_ent + 1); w /= w.sum()
    data = np.stack([rng.integers(0, n_ent, n), rng.integers(0, n_rel, n), rng.choice(n_ent, n, p=w), days * 24 + rng.integers(0, 24, n)], 1)
    data = data[np.argsort(data[:, 3], kind="stable")]
    data[10:14] = data[9]                                                        # duplicate rows stay parallel edges

    class P:
        pass

    p = P()
    p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = n_ent, n_rel, data, 24, d, a, n_layer, act, "cuda"
    torch.manual_seed(3)
    model = X.T_RED_GNN(p).cuda().eval()
    q = data[np.sort(rng.choice(np.arange(30, n), B, replace=False))]            # queries across the whole time range

    class Q:
        src_idx, rel_idx, ts = q[:, 0], q[:, 1], q[:, 3]

    with torch.no_grad():                      # (as main.py:376-384 evaluates; with gradients enabled the forward is differentiable)
        score_all, (soft, ents) = model(Q)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    otrace = []
    ref_s, ref_soft, ref_ents = orc.extrap_forward(sd, data, orc.get_time_offset_list(data, 24), 24, n_ent, n_rel, q[:, 0], q[:, 1], q[:, 3],
                                                   n_layer, act, trace=otrace)
    assert np.array_equal(ents, ref_ents)
    assert model.last_stats["n_edges"] == [t["n_edges"] for t in otrace]
    np.testing.assert_allclose(score_all.cpu().numpy(), ref_s.numpy(), rtol=RTOL, atol=ATOL_H)
    assert np.array_equal(score_all.cpu().numpy() == 0, ref_s.numpy() == 0)
    np.testing.assert_allclose(soft.cpu().numpy(), ref_soft.numpy(), rtol=2e-4, atol=1e-7)
    # the evaluation of main.py:404 on top: same ranks from either path's scores
    sp2o = {(int(s), int(r)): np.unique(data[(data[:, 0] == s) & (data[:, 1] == r), 2]) for s, r in zip(q[:, 0], q[:, 1])}
    spt2o = {(int(s), int(r), int(t)): np.unique(data[(data[:, 0] == s) & (data[:, 1] == r) & (data[:, 3] == t), 2]) for s, r, t in zip(q[:, 0], q[:, 1], q[:, 3])}
    r1 = X.segment_rank_fil(soft, ents, q[:, 2], sp2o, spt2o, q[:, 0].tolist(), q[:, 1].tolist(), q[:, 3].tolist())
    r2 = X.segment_rank_fil(ref_soft, ref_ents, q[:, 2], sp2o, spt2o, q[:, 0].tolist(), q[:, 1].tolist(), q[:, 3].tolist())
    assert r1[1] == r2[1] and np.mean(r1[0] != r2[0]) <= 0.1 and np.mean(r1[2] != r2[2]) <= 0.1       # (near-ties may swap)


def _extrap_setup(n_ent, n_rel, data, d, a, act, n_layer, seed=3):
    from red_gnn_amd import extrapolation as X

    class P:
        pass

    p = P()
    p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = n_ent, n_rel, data, 24, d, a, n_layer, act, "cuda"
    torch.manual_seed(seed)
    return X.T_RED_GNN(p).cuda()


@pytest.mark.parametrize("d,a,act,n_layer,B", [(32, 5, "tanh", 3, 9), (64, 30, "relu", 2, 24), (20, 3, "idd", 2, 3)])
def test_temporal_extrapolation_training_step_vs_oracle_autograd(d, a, act, n_layer, B):
    """SURVEY 8 f4, training (Temporal/extrapolation/main.py:296-320 around model_cuda_new_embedding.py:135-261): the windowed layer's
    adjoint rg_xlayer_bwd - scores, the loss of main.py:303-308 and the gradient of EVERY parameter the forward uses against torch
    autograd through the oracle's restatement (parity UNPINNED, as the forward: the model file cannot be imported here).  Queries
    older and younger than the window, days without rows, hub objects, duplicate rows, cut hub rows."""
    rng = np.random.default_rng(7 * d + B)
    n_ent, n_rel, n = 150, 6, 6000
    days = np.sort(rng.choice(np.delete(np.arange(220), [0, 50, 51, 120]), n))
    w = 1.0 / np.arange(1, n_ent + 1); w /= w.sum()
    data = np.stack([rng.choice(n_ent, n, p=w[::-1]), rng.integers(0, n_rel, n), rng.choice(n_ent, n, p=w), days * 24 + rng.integers(0, 24, n)], 1)
    data = data[np.argsort(data[:, 3], kind="stable")]
    data[10:14] = data[9]
    model = _extrap_setup(n_ent, n_rel, data, d, a, act, n_layer).train()
    q = data[np.sort(rng.choice(np.arange(30, n), B, replace=False))]

    class Q:
        src_idx, rel_idx, ts = q[:, 0], q[:, 1], q[:, 3]

    target = torch.as_tensor(q[:, 2], dtype=torch.long)
    score, (soft, ents) = model(Q)
    loss = F.nll_loss(torch.log(F.softmax(score, dim=1) + 1e-12), target.cuda())
    loss.backward()
    sd = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    ref_s, ref_soft, ref_ents = orc.extrap_forward(sd, data, orc.get_time_offset_list(data, 24), 24, n_ent, n_rel, q[:, 0], q[:, 1], q[:, 3], n_layer, act)
    ref_loss = F.nll_loss(torch.log(F.softmax(ref_s, dim=1) + 1e-12), target)
    ref_loss.backward()
    assert np.array_equal(ents, ref_ents)
    np.testing.assert_allclose(score.detach().cpu().numpy(), ref_s.detach().numpy(), rtol=RTOL, atol=ATOL_H)
    assert abs(loss.item() - ref_loss.item()) < 2e-5 * max(1.0, abs(ref_loss.item()))
    used = 0
    for k, v in model.named_parameters():
        ref = sd[k].grad
        if ref is None:                      # parameters the reference constructs but its forward never reads
            assert v.grad is None or not v.grad.any(), k
            continue
        used += 1
        ref = ref.numpy()
        np.testing.assert_allclose(v.grad.cpu().numpy(), ref, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(ref).max())), err_msg=k)
    assert used >= 4 * n_layer + 4
    # a second step on another batch reuses the frontier (its windows are set anew) - and an inference call in between clears them
    model.zero_grad()
    with torch.no_grad():
        model(Q)
    score2, _ = model(Q)
    assert torch.equal(score2, score)


def test_temporal_extrapolation_icews14_shape():
    """The extrapolation path at the ICEWS14 shape (7 k entities, 230 + 230 relations, 365 days of hourly stamps, 180 k time-sorted rows)
    with real 120-day windows: forward vs the oracle on queries late in the year (full windows), properties at batch size 32 (every
    query's visited set holds its subject, softmax sums to one, scores of unvisited entities are exact zeros, edge counts grow with
    the hop), and one training step with finite gradients."""
    from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape
    data, n_ent, n_rel, gran = make_extrapolation_shape("X")
    sh = SHAPES["X"]
    assert data.shape == (180_000, 4) and n_ent == 7000 and n_rel == 460 and np.all(np.diff(data[:, 3]) >= 0)
    model = _extrap_setup(n_ent, n_rel, data, sh["hidden_dim"], sh["attn_dim"], "relu", sh["n_layer"]).eval()
    rng = np.random.default_rng(5)
    late = np.flatnonzero(data[:, 3] // gran >= 200)
    q = data[np.sort(rng.choice(late, 32, replace=False))]

    class Q:
        src_idx, rel_idx, ts = q[:, 0], q[:, 1], q[:, 3]

    with torch.no_grad():
        score, (soft, ents) = model(Q)
    e = model.last_stats["n_edges"]
    assert e[0] < e[1] < e[2] and e[2] > 1e6
    b = torch.as_tensor(ents[:, 0]).cuda()
    assert torch.allclose(torch.zeros(32, device="cuda").index_add(0, b, soft), torch.ones(32, device="cuda"), atol=1e-5)
    visited = torch.zeros(32, n_ent, dtype=torch.bool)
    visited[ents[:, 0], ents[:, 1]] = True
    assert bool(visited[np.arange(32), q[:, 0]].all()) and not bool(score.cpu()[~visited].any())
    # three of the queries against the oracle (its per-query python loop over the 60 k-row windows is the slow part)
    sel = [0, 13, 31]

    class Q3:
        src_idx, rel_idx, ts = q[sel, 0], q[sel, 1], q[sel, 3]

    with torch.no_grad():
        s3, (soft3, ents3) = model(Q3)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref_s, ref_soft, ref_ents = orc.extrap_forward(sd, data, orc.get_time_offset_list(data, gran), gran, n_ent, n_rel, q[sel, 0], q[sel, 1], q[sel, 3],
                                                   sh["n_layer"], "relu")
    assert np.array_equal(ents3, ref_ents)
    ref64 = orc.extrap_forward(sd, data, orc.get_time_offset_list(data, gran), gran, n_ent, n_rel, q[sel, 0], q[sel, 1], q[sel, 3], sh["n_layer"],
                               "relu", dtype=torch.float64)[0].numpy()
    U.assert_close_fp32(s3.cpu().numpy(), ref_s.numpy(), ref64, RTOL, ATOL_H, "extrapolation scores at the ICEWS14 shape")
    # a query's scores do not depend on its batch (up to the row-chunking of the dense GEMMs, which follows the row count)
    np.testing.assert_allclose(s3.cpu().numpy(), score[sel].cpu().numpy(), rtol=1e-5, atol=1e-6)
    model.train()
    score_t, _ = model(Q)
    F.nll_loss(torch.log(F.softmax(score_t, dim=1) + 1e-12), torch.as_tensor(q[:, 2], dtype=torch.long).cuda()).backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert len(grads) >= 16 and all(torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)


def _grads(model):
    return {k: (v.grad.detach().cpu().numpy() if v.grad is not None else None) for k, v in model.named_parameters()}


def test_temporal_train_step_matches_reference_model_py_fixture():
    """A training step of T-RED-GNN (mode='train': the batch's quadruples leave the graph; rg_tlayer_fwd + rg_tlayer_bwd)
    vs scores, loss and parameter gradients of the reference's model.py + main.py:70-82."""
    fx = U.load("temporal_model_py_train.npz")
    n_layer, d, a = (int(x) for x in fx["cfg"])
    model = _temporal_model(fx, True, n_layer, d, a, str(fx["act"])).train()
    model.load_state_dict({k: torch.tensor(v) for k, v in U.params_of(fx).items()}, strict=True)
    batch = {"head": fx["heads"], "relation": fx["rels"], "time": fx["times"], "example_idx": fx["example_idx"]}
    s = model(batch, mode="train")
    np.testing.assert_allclose(s.detach().cpu().numpy(), fx["scores"], rtol=RTOL, atol=ATOL)
    loss = F.nll_loss(torch.log(F.softmax(s, dim=1) + 1e-12), torch.tensor(fx["tails"], device="cuda"))
    assert abs(loss.item() - float(fx["loss"])) < 1e-5
    loss.backward()
    for k, g in _grads(model).items():
        ref = fx["grad::" + k]
        np.testing.assert_allclose(g, ref, rtol=2e-4, atol=1e-5 * max(1.0, float(np.abs(ref).max())), err_msg=k)


@pytest.mark.parametrize("d,a,act,n_layer,B", [(64, 30, "relu", 3, 7), (32, 5, "tanh", 3, 40), (20, 30, "idd", 2, 3), (128, 16, "tanh", 2, 5)])
def test_temporal_backward_vs_oracle_autograd(d, a, act, n_layer, B):
    """Per-layer tables (model_cuda.py layout), hub rows cut into segments, sparse and dense walks: parameter gradients of a
    weighted score sum vs autograd through the oracle.  (The attention MLP's relu has a kink: an edge whose pre-activation
    rounds to the other side of 0 in one of the two implementations shifts ONE row of attention_1's gradient by that edge's
    term; the error message names the rows so such a flip is recognisable.  The seeds below have none.)"""
    rng = np.random.default_rng(5)
    n_ent, n_rel, n_time, n_q = 300, 9, 365, 4000
    w = 1.0 / np.arange(1, n_ent + 1); w /= w.sum()
    h, t = rng.choice(n_ent, n_q, p=w), rng.integers(0, n_ent, n_q)
    quads = np.stack([h, rng.integers(0, n_rel - 1, n_q), t, rng.integers(0, n_time - 1, n_q)], 1)
    quads[:100, 3] = quads[100:200, 3]
    idd = np.stack([np.arange(n_ent), np.full(n_ent, n_rel - 1), np.arange(n_ent), np.full(n_ent, n_time - 1)], 1)
    full = np.concatenate([quads, quads[:, [2, 1, 0, 3]], idd], 0).astype(np.int32)
    fx = dict(quads=full, n_ent=n_ent, n_rel=n_rel, n_time=n_time)
    model = _temporal_model(fx, False, n_layer, d, a, act, seed=11).train()
    ex = rng.choice(n_q, B, replace=False)
    batch = {"head": quads[ex, 0], "relation": quads[ex, 1], "time": quads[ex, 3], "example_idx": ex}
    weight = torch.tensor(rng.standard_normal((B, n_ent)), dtype=torch.float32)
    s = model(batch, mode="train")
    (s * weight.cuda()).sum().backward()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    ref = orc.temporal_forward(p, np.delete(full, ex, axis=0), n_ent, batch["head"], batch["relation"], batch["time"], n_layer, act)
    np.testing.assert_allclose(s.detach().cpu().numpy(), ref.detach().numpy(), rtol=RTOL, atol=ATOL_H)
    (ref * weight).sum().backward()
    for k, g in _grads(model).items():
        if p[k].grad is None:
            assert g is None or not np.any(g), k          # score_embed_layer / query_relation_linear: unused by the forward
            continue
        r = p[k].grad.numpy()
        atol = 2e-5 * max(1.0, float(np.abs(r).max()))
        bad = np.argwhere(~np.isclose(g, r, rtol=2e-3, atol=atol))
        np.testing.assert_allclose(g, r, rtol=2e-3, atol=atol, err_msg="%s rows %s cols %s" % (k, np.unique(bad[:, 0]), np.unique(bad[:, -1])))


# ---- edge cases ------------------------------------------------------------------------------------------------
def _ids(n_ent, n_rel, facts, train=None, test=None):
    z = np.zeros((0, 3), np.int64)
    return dict(n_ent=n_ent, n_rel=n_rel, facts=np.asarray(facts, np.int64).reshape(-1, 3),
                train=z if train is None else np.asarray(train, np.int64).reshape(-1, 3), valid=z,
                test=z if test is None else np.asarray(test, np.int64).reshape(-1, 3))


@pytest.mark.parametrize("case", ["tiny", "hubs", "C2", "C3", "no_triples", "wide_ent", "wide_rel"])
def test_device_graph_build_equals_host_build(case):
    """rg_graph_create_device (the graph of shuffle_train's re-split, built where it is used) against rg_graph_create on the same
    triples: both CSRs, the length-sorted virtual rows and the word-parallel walk's packs are equal array for array; the model
    gives bitwise the same scores on either."""
    from red_gnn_amd.engine import Graph
    from red_gnn_amd.synthetic import make_shape, make_synthetic_kg
    rng = np.random.default_rng(5)
    if case in ("C2", "C3"):
        kg = make_shape(case)
        n_ent, n_rel, trip = kg.n_ent, kg.n_rel, np.concatenate([kg.facts, kg.train], 0)
    elif case == "no_triples":
        n_ent, n_rel, trip = 37, 2, np.zeros((0, 3), np.int64)
    elif case in ("wide_ent", "wide_rel"):
        # ids too wide for the packed (rel << 20 | entity) entries (graph.hip: n_ent <= 2^20 && n_rela_rows <= 2^12): int2 entries only,
        # no word-parallel packs; the highest entity ids and relation ids are in use
        n_ent, n_rel, m = ((1 << 20) + 37, 5, 5000) if case == "wide_ent" else (700, 2050, 5000)
        h, t = rng.integers(0, n_ent, m), rng.integers(0, n_ent, m)
        h[:40], t[40:80] = n_ent - 1 - np.arange(40), n_ent - 1 - np.arange(40)
        r = rng.integers(0, n_rel, m)
        r[:3] = n_rel - 1
        trip = np.stack([h, r, t], 1)
    else:
        n_ent, n_rel, m = (50, 4, 300) if case == "tiny" else (400, 7, 9000)
        h, t = rng.integers(0, n_ent, m), rng.integers(0, n_ent, m)
        if case == "hubs":
            t[: m // 3] = 11                      # an in-row cut into > 20 segments
            h[m // 3: m // 2] = 5                 # an out-row cut into segments
        trip = np.stack([h, rng.integers(0, n_rel, m), t], 1)
        trip = np.concatenate([trip, trip[:7]], 0)                     # duplicates stay parallel edges
    trip = trip[rng.permutation(len(trip))]
    g_h = Graph(n_ent, n_rel, trip)
    g_d = Graph.from_device(n_ent, n_rel, torch.as_tensor(trip, dtype=torch.int32).cuda())
    assert g_h.n_fact == g_d.n_fact == 2 * len(trip) + n_ent
    for a, b, name in zip(g_h.export(), g_d.export(), ("out_ptr", "out_rel_tail", "in_ptr", "in_head_rel")):
        assert np.array_equal(a, b), name
    for a, b, name in zip(g_h.export_packs(), g_d.export_packs(), ("in_vrows", "pack_entries", "packs", "pack_rows")):
        assert a.shape == b.shape and np.array_equal(a, b), name
    assert (len(g_h.export_packs()[2]) == 0) == case.startswith("wide_")      # int2 entries only: no word-parallel packs


def test_shuffle_train_builds_its_graph_on_the_device():
    """DataLoader.shuffle_train (load_data.py:152-164): same split as the reference's formula for the same numpy seed, the training
    graph (built by rg_graph_create_device from the resident triples) equals the host build of that split, and training-mode
    forwards on it match the oracle on the re-split facts."""
    from red_gnn_amd.engine import Graph
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(300, 5, 3000, seed=23)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 2, 32, 5, "relu", seed=6)
    allt = np.concatenate([kg.facts, kg.train], 0)
    for epoch in range(2):                                     # every epoch permutes the ORIGINAL concatenation (the reference keeps it)
        np.random.seed(100 + epoch)
        loader.shuffle_train()
        np.random.seed(100 + epoch)
        perm = np.random.permutation(len(allt))
        facts, train = allt[perm][: len(allt) * 3 // 4], allt[perm][len(allt) * 3 // 4:]
        assert np.array_equal(loader.train_data, orc.double_triple(train, kg.n_rel))
        assert np.array_equal(loader.fact_data, orc.double_triple(facts, kg.n_rel))
        g_ref = Graph(kg.n_ent, kg.n_rel, facts)
        for a, b in zip(loader.graph.export(), g_ref.export()):
            assert np.array_equal(a, b)
        trip = loader.train_data[:9]
        with torch.no_grad():
            s = model(trip[:, 0], trip[:, 1], mode="train").cpu().numpy()
        p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        og = orc.OracleGraph(orc.double_triple(facts, kg.n_rel), kg.n_ent, kg.n_rel)
        ref = orc.forward(p, og, trip[:, 0], trip[:, 1], 2, act="relu").numpy()
        np.testing.assert_allclose(s, ref, rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("n_ent,B", [(1, 1), (31, 1), (33, 3), (64, 33), (97, 65)])
def test_edge_shapes_vs_oracle(n_ent, B):
    """n_ent / batch sizes around the 32-bit word and 64-lane boundaries, isolated entities (identity edge only),
    duplicate triples (kept as parallel edges, SURVEY §8 a4'), a graph with no triples at all (n_ent = 1)."""
    from red_gnn_amd.load_data import DataLoader
    rng = np.random.default_rng(n_ent * 131 + B)
    n_rel = 3
    m = 0 if n_ent == 1 else 4 * n_ent
    h, t = rng.integers(0, max(n_ent - 2, 1), m), rng.integers(0, max(n_ent - 2, 1), m)     # the last entities stay isolated
    facts = np.stack([h, rng.integers(0, n_rel, m), t], 1).reshape(-1, 3)
    if m:
        facts = np.concatenate([facts, facts[:5]], 0)                                        # duplicates
    ids = _ids(n_ent, n_rel, facts)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, 32, 5, "relu", seed=3)
    subs = rng.integers(0, n_ent, B)
    subs[-1] = n_ent - 1                                                                     # an isolated query subject
    rels = rng.integers(0, 2 * n_rel, B)
    trace, otrace = [], []
    with torch.no_grad():
        s = model(subs, rels, mode="test", trace=trace).cpu().numpy()
    p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = orc.forward(p, U.oracle_graph(ids, "test"), subs, rels, 3, act="relu", trace=otrace).numpy()
    for a, b in zip(trace, otrace):
        assert np.array_equal(a["nodes"].cpu().numpy(), b["nodes"])
        assert a["n_edges"] == len(b["edges"])
    np.testing.assert_allclose(s, ref, rtol=RTOL, atol=ATOL)
    assert np.array_equal(s == 0, ref == 0)
    # the same through the reference-compatible get_neighbors, hop by hop, incl. duplicated edges
    nodes = np.stack([np.arange(B), subs], 1)
    og = U.oracle_graph(ids, "test")
    for _ in range(2):
        t_nodes, t_edges, t_old = orc.get_neighbors(og, nodes)
        g_nodes, g_edges, g_old = loader.get_neighbors(nodes, mode="test")
        assert np.array_equal(g_nodes.cpu().numpy(), t_nodes) and np.array_equal(g_old.cpu().numpy(), t_old)
        assert np.array_equal(U.sorted_edges(g_edges.cpu().numpy()), U.sorted_edges(t_edges))
        nodes = t_nodes


def test_bad_inputs_raise():
    from red_gnn_amd import _lib
    from red_gnn_amd import engine as engine_mod
    from red_gnn_amd.load_data import DataLoader
    ids = _ids(10, 2, [[0, 0, 1], [1, 1, 2]])
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 2, 16, 3, "relu")
    with pytest.raises(ValueError):
        model(np.array([0, 10]), np.array([0, 1]), mode="test")          # subject id == n_ent (checked on the host)
    fr = engine_mod.Frontier(10, 2, 2, "cuda")
    fr.reset(torch.tensor([0, 10], dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.NativeError):
        fr.expand(loader.graph_for("test"))                              # ... and by the library when it gets that far
    with pytest.raises(_lib.NativeError):
        loader.get_neighbors(np.array([[0, 1], [0, 1]]), mode="test")    # duplicate start nodes
    with pytest.raises(_lib.NativeError):
        DataLoader(ids=_ids(10, 2, [[0, 5, 1]]), verbose=False).graph    # relation id out of range
    s = model(np.array([0, 9]), np.array([0, 3]), mode="test")           # still usable after the errors
    assert torch.isfinite(s).all()


def test_large_batch_property_checksum():
    """BASELINE-size check without the oracle: sum over queries of scores is invariant to the order of the queries in
    the batch (per-query independence + deterministic per-destination sums), B = 512 on C2."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_shape
    kg = make_shape("C2")
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 3, 64, 5, "relu")
    B = 512
    subs, rels = kg.test[:B, 0], kg.test[:B, 1]
    perm = np.random.default_rng(0).permutation(B)
    with torch.no_grad():
        s1 = model(subs, rels, mode="test")
        s2 = model(subs[perm], rels[perm], mode="test")
    np.testing.assert_allclose(s2.cpu().numpy(), s1[perm].cpu().numpy(), rtol=RTOL, atol=ATOL)
    assert torch.equal(s2 == 0, s1[perm] == 0)


def test_five_adam_steps_track_the_oracle():
    """Drop-in check of the whole training step: 5 x (forward, the reference's loss, HIP backward, Adam) with
    dropout 0 leave the parameters where the same steps through the oracle (CPU autograd) leave them."""
    from red_gnn_amd.base_model import reference_loss
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(300, 5, 2500, seed=17)
    ids = dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)
    loader = DataLoader(ids=ids, verbose=False)
    torch.manual_seed(3)
    model = RED_GNN_trans(P(3, 32, 5, loader.n_rel, "relu"), loader).cuda().train()
    ref = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, weight_decay=1e-5)
    ropt = torch.optim.Adam(list(ref.values()), lr=2e-3, weight_decay=1e-5)
    og = U.oracle_graph(ids, "train")
    for step in range(5):
        trip = loader.train_data[step * 10:(step + 1) * 10]
        opt.zero_grad()
        loss = reference_loss(model(trip[:, 0], trip[:, 1]), torch.as_tensor(trip[:, 2], device="cuda"))
        loss.backward()
        opt.step()
        ropt.zero_grad()
        rloss = orc.loss_fn(orc.forward(ref, og, trip[:, 0], trip[:, 1], 3, act="relu"), trip[:, 2])
        rloss.backward()
        ropt.step()
        assert abs(loss.item() - rloss.item()) < 2e-3 * abs(rloss.item()), (step, loss.item(), rloss.item())
    for k, v in model.named_parameters():
        np.testing.assert_allclose(v.detach().cpu().numpy(), ref[k].detach().numpy(), rtol=5e-3, atol=2e-4, err_msg=k)


def test_random_graphs_fuzz_vs_oracle():
    """Forty small random graphs / batches / widths in one process: node sets bit-exact, scores within tolerance.
    Catches indexing mistakes that fixed shapes miss (segment boundaries at 128, word boundaries, empty frontiers)."""
    from red_gnn_amd.load_data import DataLoader
    rng = np.random.default_rng(2024)
    for case in range(int(os.environ.get("RG_FUZZ_N", "40"))):
        n_ent = int(rng.integers(2, 400))
        n_rel = int(rng.integers(1, 9))
        m = int(rng.integers(0, 12 * n_ent))
        hub = int(rng.integers(0, n_ent))
        h, t = rng.integers(0, n_ent, m), rng.integers(0, n_ent, m)
        if case % 3 == 0 and m:
            t[: m // 2] = hub                      # one hub with an in-row cut into segments
        if case % 5 == 0 and m:
            h[m // 2:] = hub
        facts = np.stack([h, rng.integers(0, n_rel, m), t], 1).reshape(-1, 3)
        ids = _ids(n_ent, n_rel, facts[: (3 * m) // 4], train=facts[(3 * m) // 4:])
        loader = DataLoader(ids=ids, verbose=False)
        d = int(rng.choice([16, 20, 32, 48, 64, 128]))
        a = int(rng.choice([3, 5, 8]))
        n_layer = int(rng.integers(1, 5))
        act = str(rng.choice(["relu", "tanh", "idd"]))
        model = _random_model(loader, n_layer, d, a, act, seed=case)
        B = int(rng.integers(1, 40))
        subs, rels = rng.integers(0, n_ent, B), rng.integers(0, 2 * n_rel, B)
        mode = "train" if case % 2 else "test"
        trace, otrace = [], []
        with torch.no_grad():
            s = model(subs, rels, mode=mode, trace=trace).cpu().numpy()
        p = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        ref = orc.forward(p, U.oracle_graph(ids, mode), subs, rels, n_layer, act=act, trace=otrace).numpy()
        for x, y in zip(trace, otrace):
            assert np.array_equal(x["nodes"].cpu().numpy(), y["nodes"]), case
            assert x["n_edges"] == len(y["edges"]), case
        np.testing.assert_allclose(s, ref, rtol=RTOL, atol=ATOL_H, err_msg="case %d" % case)
        assert np.array_equal(s == 0, ref == 0), case
        if case % 2 == 0:           # the same forward as a replayed HIP graph (third call of the shape): bit-identical
            with torch.no_grad():
                for _ in range(3):
                    s3 = model(subs, rels, mode=mode)
            assert len(model._graphed) == 1 and np.array_equal(s3.cpu().numpy(), s), case


def test_evaluation_lanes_give_the_same_metrics():
    """BaseModel.evaluate deals batches to EVAL_LANES streams (each replaying its own captured forward): ranks - and so MRR / H@k -
    are identical to the single-stream evaluation, pass after pass (eager warm-up calls, captures and replays included)."""
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    ids = U.load("family_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class Opt:
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch, n_tbatch = 0.0036, 0.999, 1.7e-5, 32, 5, 3, 0.1, "relu", 20, 50
        n_rel = loader.n_rel

    torch.manual_seed(7)
    bm = BaseModel(Opt, loader)
    bm.n_valid, bm.n_test = 620, 415                      # 13 + 9 batches, both with a partial last batch
    bm.model.eval()
    saved = BaseModel.EVAL_LANES
    try:
        BaseModel.EVAL_LANES = 1
        ref_v = bm._rank_split("valid", bm.n_valid).cpu().numpy()
        ref_t = bm._rank_split("test", bm.n_test).cpu().numpy()
        BaseModel.EVAL_LANES = 16
        for _ in range(4):                                  # warm-up (eager), capture, replays
            assert np.array_equal(bm._rank_split("valid", bm.n_valid).cpu().numpy(), ref_v)
            assert np.array_equal(bm._rank_split("test", bm.n_test).cpu().numpy(), ref_t)
    finally:
        BaseModel.EVAL_LANES = saved
    assert len(bm.model._graphed) >= 8


def test_evaluation_batches_fused_per_pass_give_the_same_scores_and_ranks():
    """BaseModel.eval_coalesce = k evaluates k reference batches of n_tbatch as one forward pass: a query's scores do not depend on the
    other queries of its batch, so the scores are the same BIT FOR BIT and the ranks identical (partial last batches included)."""
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    ids = U.load("family_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class Opt:
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch, n_tbatch = 0.0036, 0.999, 1.7e-5, 64, 5, 3, 0.1, "relu", 20, 50
        n_rel = loader.n_rel

    torch.manual_seed(11)
    bm = BaseModel(Opt, loader)
    bm.n_valid = 430                                      # 8 full batches and one of 30
    bm.model.eval()
    ref = bm._rank_split("valid", bm.n_valid).cpu().numpy()
    for k in (3, 4):
        bm.eval_coalesce = k
        for _ in range(3):                                # eager, capture, replay
            assert np.array_equal(bm._rank_split("valid", bm.n_valid).cpu().numpy(), ref), k
    # scores of the first 200 queries: four passes of 50 against one of 200
    with torch.no_grad():
        parts = [bm.model(*loader.get_batch_csr(np.arange(i, i + 50), data="valid")[:2], mode="valid") for i in range(0, 200, 50)]
        whole = bm.model(*loader.get_batch_csr(np.arange(200), data="valid")[:2], mode="valid")
    assert torch.equal(torch.cat(parts), whole)


def test_inductive_training_learns():
    """The reference's loop in the inductive setting (train on the transductive graph's valid triples, evaluate the
    'test' split on the inductive graph with its own entity set): one short epoch lifts the inductive MRR."""
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    ids = U.load("ind_WN18RR_v1_ids.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class Opt:      # Static/inductive/train.py WN18RR_v1 preset
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch, n_tbatch = 0.005, 0.991, 0.0002, 64, 5, 5, 0.21, "relu", 100, 100
        n_rel = loader.n_rel

    np.random.seed(1234)
    torch.manual_seed(1234)
    bm = BaseModel(Opt, loader)
    assert isinstance(bm.model, RED_GNN_induc)
    bm.model.eval()
    from red_gnn_amd.utils import cal_performance
    mrr0 = bm._performance(bm._rank_split("test", bm.n_test))[0]
    for epoch in range(3):
        v_mrr, out = bm.train_batch(epoch=epoch)
    t_mrr = float(out.split("[TEST] MRR:")[1].split()[0])
    assert np.isfinite(bm.last_epoch_loss) and t_mrr > max(0.3, 2 * mrr0), (mrr0, out)


def test_two_rank_training_matches_single_process():
    """SURVEY §8e on the trainer: two processes (gloo, sharing this GPU) shard every batch by query, all-reduce gradients
    and metric sums; parameters stay identical across ranks and track the single-process run (tools/dist_train_check.py)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "tools", "dist_train_check.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0 and "DIST_TRAIN_CHECK_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def test_nan_scrub_replaces_only_nans_and_consumes_one_draw_per_parameter():
    """base_model.py:64-69 of the reference: X[np.isnan(X)] = np.random.random() for every parameter after each step."""
    from red_gnn_amd.base_model import BaseModel
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(60, 4, 400, seed=2)
    loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test), verbose=False)

    class Opt:
        lr, decay_rate, lamb, hidden_dim, attn_dim, n_layer, dropout, act, n_batch, n_tbatch = 0.01, 0.99, 1e-5, 16, 3, 2, 0.0, "relu", 8, 8
        n_rel = loader.n_rel

    bm = BaseModel(Opt, loader)
    params = list(bm.model.parameters())
    with torch.no_grad():
        params[0].data[0, 0] = float("nan")
        params[0].data[0, 1] = float("inf")
        params[3].data.view(-1)[2] = float("nan")
    before = [p.detach().clone() for p in params]
    np.random.seed(99)
    draws = [np.random.random() for _ in params]
    np.random.seed(99)
    bm._scrub_nan()
    assert np.random.random() == np.random.RandomState(99).random_sample(len(params) + 1)[-1]      # one draw per parameter
    assert params[0].data[0, 0].item() == pytest.approx(draws[0]) and params[0].data[0, 1].item() == float("inf")
    assert params[3].data.view(-1)[2].item() == pytest.approx(draws[3])
    for p, b in zip(params, before):
        keep = ~torch.isnan(b)
        assert torch.equal(p.data[keep], b[keep])


def test_graph_replay_matches_eager_forward():
    """Inference as a captured HIP graph (rg_frontier_expand_async + rg_dense_fwd_dev, buffers at full-grid capacity): from the
    third call of a shape on the forward is a graph replay; scores, stats and ranks equal the eager path's bit for bit, for
    changing queries and after a parameter update."""
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(500, 9, 6000, seed=8)
    loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test), verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 3, 48, 5, kg.n_rel, "relu", 0.1

    torch.manual_seed(3)
    model = RED_GNN_trans(P, loader).cuda().eval()
    rng = np.random.default_rng(0)
    B = 37
    with torch.no_grad():
        for it in range(6):
            q = kg.test[rng.integers(0, len(kg.test), B)]
            model.use_graphs = True
            s_g = model(q[:, 0], q[:, 1], mode="test")
            st_g = dict(model.last_stats)
            model.use_graphs = False
            s_e = model(q[:, 0], q[:, 1], mode="test")
            st_e = dict(model.last_stats)
            assert torch.equal(s_g, s_e), it
            assert st_g == st_e, (it, st_g, st_e)
            if it == 3:                                       # parameters change in place between replays (training between evals)
                for p_ in model.parameters():
                    p_.data.mul_(1.01)
    assert len(model._graphed) == 1


@pytest.mark.parametrize("d,prec", [(64, "f32"), (64, "f16x2"), (24, "f16x2"), (64, "f16x3"), (48, "f16x3"), (24, "f16x3"), (128, "f32"), (128, "f16x2"), (128, "f16x3")])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 127, 128, 129, 1000, 4099])
def test_dense_kernel_row_count_edges(d, prec, n):
    """rg_dense_fwd / rg_dense_fwd_dev straight through the engine on row counts around the 16-node tile and the 128-node round
    of the streamed d=128 kernel, with and without old nodes, middle layer (a_s out) and last layer (readout), against torch."""
    from red_gnn_amd import engine
    torch.manual_seed(n * 7 + d)
    a, ap, n_old, n_ent = 5, 8, max(1, n // 3), 50
    dev = "cuda"
    agg = torch.randn(n, d, device=dev)
    hprev = torch.randn(n_old, d, device=dev)
    prev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    sel = torch.randperm(n, device=dev)[:min(n_old, n)]
    prev[sel] = torch.arange(sel.numel(), dtype=torch.int32, device=dev)
    gate = torch.nn.GRU(d, d).to(dev)
    W_h, Ws, W_final = torch.randn(d, d, device=dev) / d ** 0.5, torch.randn(a, d, device=dev) / d ** 0.5, torch.randn(1, d, device=dev)
    nodes = torch.stack([torch.arange(n, device=dev, dtype=torch.int32) // n_ent, torch.arange(n, device=dev, dtype=torch.int32) % n_ent], 1).contiguous()
    n_q = (n + n_ent - 1) // n_ent

    def reference(prev_idx):
        x = torch.tanh(agg @ W_h.t())
        h0 = torch.zeros(n, d, device=dev)
        if prev_idx is not None:
            m = prev_idx >= 0
            h0[m] = hprev[prev_idx[m].long()]
        h = torch.gru_cell(x, h0, gate.weight_ih_l0, gate.weight_hh_l0, gate.bias_ih_l0, gate.bias_hh_l0)
        return h, h @ Ws.t(), (h @ W_final.t()).reshape(-1)

    with torch.no_grad():
        for prev_idx in (prev, None):
            h_ref, as_ref, sc_ref = reference(prev_idx)
            h1, a1 = engine.dense_fwd(agg, hprev, prev_idx, d, W_h, "tanh", gate, Ws_next=Ws, attn_dim=a, ap=ap, precision=prec)
            np.testing.assert_allclose(h1.cpu().numpy(), h_ref.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
            np.testing.assert_allclose(a1[:, :a].cpu().numpy(), as_ref.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
            scores = torch.zeros(n_q * n_ent, device=dev)
            h2, _ = engine.dense_fwd(agg, hprev, prev_idx, d, W_h, "tanh", gate, W_final=W_final, nodes=nodes, n_ent=n_ent, scores_all=scores,
                                     precision=prec)
            assert torch.equal(h1, h2)
            np.testing.assert_allclose(scores[:n].cpu().numpy(), sc_ref.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
            assert not scores[n:].any()
        # the device-count form on buffers with spare capacity: rows beyond the count stay untouched
        cap = n + 300
        agg_c = torch.cat([agg, torch.full((300, d), float("nan"), device=dev)])
        prev_c = torch.cat([prev, torch.full((300,), 5, dtype=torch.int32, device=dev)])
        out = torch.full((cap, d), -7.0, device=dev)
        a_out = torch.full((cap, ap), -7.0, device=dev)
        count = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device=dev)
        import ctypes
        engine.dense_fwd_dev(cap, ctypes.c_void_p(count.data_ptr()), agg_c, hprev, prev_c, d, W_h, "tanh", gate, out, Ws_next=Ws, attn_dim=a,
                             ap=ap, a_s_out=a_out, precision=prec)
        h_ref, as_ref, _ = reference(prev)
        np.testing.assert_allclose(out[:n].cpu().numpy(), h_ref.cpu().numpy(), rtol=RTOL, atol=ATOL_H)
        assert bool((out[n:] == -7.0).all()) and bool((a_out[n:] == -7.0).all())
        # n_hint only sizes the grid: far too small an expectation still processes every row
        out2 = torch.full((cap, d), -7.0, device=dev)
        engine.dense_fwd_dev(cap, ctypes.c_void_p(count.data_ptr()), agg_c, hprev, prev_c, d, W_h, "tanh", gate, out2, Ws_next=Ws, attn_dim=a,
                             ap=ap, a_s_out=a_out, n_hint=max(1, n // 7), precision=prec)
        assert torch.equal(out2, out)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("scale", [1e-6, 1e-3, 1.0, 300.0])
def test_split_dense_kernel_fits_its_weight_scale(scale, d):
    """The f16-split dense kernel stages all weights under one power-of-two scale: 2^12 by default, refitted in a second staging pass
    when the weights' largest magnitude would overflow f16 or leave the lo halves denormal.  Both paths against fp64, at the same
    tolerance as unit-scale weights (relative to each output's magnitude)."""
    from red_gnn_amd import engine
    torch.manual_seed(11)
    dev, n, a, ap = "cuda", 3000, 5, 8
    agg = torch.randn(n, d, device=dev)
    hprev = torch.tanh(torch.randn(n // 2, d, device=dev))
    prev = torch.randint(-1, n // 2, (n,), device=dev, dtype=torch.int32)
    gate = torch.nn.GRU(d, d).to(dev)
    small = min(scale, 1.0)        # (large gate weights saturate the gates and make the comparison ill-conditioned: the large case
    with torch.no_grad():          # scales the projection only, which is enough to push the largest weight past the default scale)
        for p_ in gate.parameters():
            p_.mul_(small)
    W_h = torch.randn(d, d, device=dev) / d ** 0.5 * small
    Ws = torch.randn(a, d, device=dev) / d ** 0.5 * scale
    f = lambda t: t.double()
    with torch.no_grad():
        x = f(agg) @ f(W_h).t()
        h0 = torch.zeros(n, d, device=dev, dtype=torch.float64)
        m = prev >= 0
        h0[m] = f(hprev)[prev[m].long()]
        gi = x @ f(gate.weight_ih_l0).t() + f(gate.bias_ih_l0)
        gh = h0 @ f(gate.weight_hh_l0).t() + f(gate.bias_hh_l0)
        r, z = torch.sigmoid(gi[:, :d] + gh[:, :d]), torch.sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
        h_ref = (1 - z) * torch.tanh(gi[:, 2 * d:] + r * gh[:, 2 * d:]) + z * h0
        as_ref = h_ref @ f(Ws).t()
        for prec in ("f16x3", "f16x2", "f32"):
            h, a_s = engine.dense_fwd(agg, hprev, prev, d, W_h, "idd", gate, Ws_next=Ws, attn_dim=a, ap=ap, precision=prec)
            assert float((h.double() - h_ref).abs().max()) < 2e-6 * max(1.0, float(h_ref.abs().max())), (prec, scale)
            assert float((a_s[:, :a].double() - as_ref).abs().max()) < 2e-6 * max(scale, float(as_ref.abs().max())), (prec, scale)


@pytest.mark.parametrize("n_rows,m,n", [(200_000, 192, 64), (70_001, 144, 48), (33_000, 64, 64), (40_000, 8, 64), (5, 192, 64), (100_003, 384, 128), (50_000, 60, 20)])
def test_gram_tn_weight_gradient_kernel(n_rows, m, n):
    """rg_gram_tn: out = G^T X and the column sums of G over node rows (the weight / bias gradients of the dense training step) against
    fp64, for every width the presets use (d = 64: 192 x 64; d = 48: 144 x 48; the attention projection: 8 x 64; d = 128 tiled over
    column blocks; widths that are no multiple of 16), on strided column blocks of wider buffers, ragged row counts, and twice: the
    sums are bitwise reproducible."""
    from red_gnn_amd import engine
    torch.manual_seed(n_rows % 97)
    dev = "cuda"
    gbuf = torch.randn(n_rows, m + 24, device=dev)
    xbuf = torch.randn(n_rows, n + 8, device=dev)
    g, x = gbuf[:, 8:8 + m], xbuf[:, 4:4 + n]            # column blocks: rows are spaced, columns unit-stride
    out, cs = engine.gram_tn(g, x, colsum=True)
    ref = g.double().t() @ x.double()
    scale = float(ref.abs().max())
    assert float((out.double() - ref).abs().max()) <= 2e-6 * max(scale, (n_rows ** 0.5))
    assert float((cs.double() - g.double().sum(0)).abs().max()) <= 2e-6 * max(float(g.double().sum(0).abs().max()), n_rows ** 0.5)
    out2, cs2 = engine.gram_tn(g, x, colsum=True)
    assert torch.equal(out, out2) and torch.equal(cs, cs2)
    assert torch.equal(engine.gram_tn(g, x), out)         # the product does not depend on the column-sum option


def _split3_roundtrip(x, parts=False):
    import ctypes
    from red_gnn_amd import _lib
    back = torch.empty_like(x)
    pt = torch.empty(x.shape + (4,), device=x.device) if parts else None
    _lib.check(_lib.lib().rg_split3_roundtrip(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(back), _lib.ptr(pt), _lib.stream_ptr()))
    return back, pt


@pytest.mark.parametrize("cols", [64, 48, 20, 128])
def test_split3_reconstructs_fp32_bit_exactly(cols):
    """precision "f16x3" carries every fp32 operand as hi + mid + lo (three f16): the device split (the kernels' own code,
    csrc/split3.h, with their row scaling) must give back the fp32 input BIT FOR BIT - random normal rows at row scales from 1e-6 to
    300 (the range test_split_dense_kernel_fits_its_weight_scale covers), uniform rows, rows of fp32 values with all 24 mantissa
    bits set, and the bf8 image of lo (the weights' form) must equal lo."""
    torch.manual_seed(3)
    dev = "cuda"
    rows = []
    for scale in (1e-6, 1e-3, 0.03, 1.0, 17.0, 300.0):
        rows.append(torch.randn(4096, cols, device=dev) * scale)
        rows.append((torch.rand(4096, cols, device=dev) * 2 - 1) * scale)
    full = torch.randint(1 << 23, 1 << 24, (4096, cols), device=dev, dtype=torch.int32)            # 1.xxx with random mantissas ...
    full = ((full | 1).float() * 2.0 ** -23) * (torch.randint(0, 2, (4096, cols), device=dev) * 2 - 1)   # ... last bit set, random sign
    rows.append(full)
    rows.append(full * 2.0 ** torch.randint(-12, 1, (4096, cols), device=dev).float())             # and 12 binades of spread inside a row
    x = torch.cat(rows)
    back, parts = _split3_roundtrip(x, parts=True)
    rowmax = x.abs().max(1, keepdim=True).values
    inside = x.abs() >= rowmax * 2.0 ** -15           # f16's range below the row scale: ~1e-4 of the random normal elements fall out of it
    assert float(inside.float().mean()) > 0.999
    assert torch.equal(back.view(torch.int32)[inside], x.view(torch.int32)[inside])
    assert bool(((back - x).abs() <= rowmax * 2.0 ** -39).all())
    assert torch.equal(back[-8192:].view(torch.int32), x[-8192:].view(torch.int32))      # the all-24-bit rows: every element
    hi, mid, lo, lo8 = parts.unbind(-1)
    assert torch.equal(lo8, lo)                                          # one significant bit: exact in bf8
    # every part is an f16 value, and the parts are non-overlapping: |mid| <= ulp(hi) / 2, |lo| <= ulp(mid) / 2
    assert torch.equal(hi.half().float(), hi) and torch.equal(mid.half().float(), mid) and torch.equal(lo.half().float(), lo)
    nz = hi != 0
    assert bool((mid.abs()[nz] <= hi.abs()[nz] * 2.0 ** -10).all()) and bool((lo.abs()[nz] <= hi.abs()[nz] * 2.0 ** -21).all())


def test_split3_small_elements_bound():
    """Elements far below their row's largest magnitude run out of f16 range (its smallest subnormal is 2^-24 at a row scale of 2^14 ..
    2^15): exact down to 2^-15 of the row's largest, then an absolute error of at most 2^-39 of the row's largest - 2^-15 of one ulp of
    the values that dominate any dot product with the row."""
    torch.manual_seed(4)
    dev = "cuda"
    x = torch.randn(2048, 64, device=dev) * 10.0 ** torch.empty(2048, 64, device=dev).uniform_(-12, 0)
    back, _ = _split3_roundtrip(x)
    rowmax = x.abs().max(1, keepdim=True).values
    big = x.abs() >= rowmax * 2.0 ** -15
    assert 0.2 < float(big.float().mean()) < 0.8
    assert torch.equal(back[big], x[big])
    assert bool(((back - x).abs() <= rowmax * 2.0 ** -39).all())


@pytest.mark.parametrize("d", [64, 48, 32])
def test_split3_products_are_exact_on_one_hot_operands(d):
    """All six partial products of the three-term kernel, through the kernel itself (rg_split3_product_check): with one-hot operand
    rows times powers of two, W x is a column of W times that power - one term per output, no summation error - and must come out
    BIT FOR BIT for weights with all 24 mantissa bits in use.  which = 1: act(W_h agg), 2: W_in x, 3: W_hn h0."""
    from red_gnn_amd import _lib
    torch.manual_seed(8)
    dev, n = "cuda", 4 * d + 37

    def full24(*shape):        # fp32 values with random 24-bit mantissas (last bit set), random signs, five binades
        m = (torch.randint(1 << 23, 1 << 24, shape, device=dev, dtype=torch.int32) | 1).float() * 2.0 ** -24
        return m * (torch.randint(0, 2, shape, device=dev) * 2 - 1).float() * 2.0 ** torch.randint(-4, 1, shape, device=dev).float()

    W_h, w_ih, w_hh = full24(d, d), full24(3 * d, d), full24(3 * d, d)
    b = torch.zeros(3 * d, device=dev)
    k = torch.arange(n, device=dev) % d
    pw = 2.0 ** (torch.arange(n, device=dev) % 7 - 3).float()
    onehot = torch.zeros(n, d, device=dev)
    onehot[torch.arange(n, device=dev), k] = pw
    prev = torch.arange(n, device=dev, dtype=torch.int32)
    eye = torch.eye(d, device=dev)
    out = torch.empty(n, d, device=dev)

    def run(which, agg, W):
        _lib.check(_lib.lib().rg_split3_product_check(which, n, d, _lib.ptr(agg), _lib.ptr(onehot), _lib.ptr(prev), _lib.ptr(W), 0,
                                                      _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(b), _lib.ptr(b), _lib.ptr(out), _lib.stream_ptr()))
        return out.clone()

    want = lambda W: (W.t()[k] * pw[:, None])
    assert torch.equal(run(1, onehot, W_h).view(torch.int32), want(W_h).view(torch.int32))
    assert torch.equal(run(2, onehot, eye).view(torch.int32), want(w_ih[2 * d:]).view(torch.int32))      # x = I agg = the one-hot rows
    assert torch.equal(run(3, onehot, eye).view(torch.int32), want(w_hh[2 * d:]).view(torch.int32))
    # and a dense operand: against fp64 the error is that of an fp32 accumulation chain (products exact)
    agg = torch.randn(n, d, device=dev)
    ref = agg.double() @ W_h.double().t()
    err = float((run(1, agg, W_h).double() - ref).abs().max() / ref.abs().max())
    assert err < 3e-7, err


@pytest.mark.parametrize("act", ["idd", "relu", "tanh"])
@pytest.mark.parametrize("d", [64, 48])
def test_split3_dense_error_not_above_exact_f32_kernel(d, act):
    """Done-criterion of the three-term kernel: measured against an fp64 evaluation of the same layer, its error is not above the
    exact-fp32 MFMA kernel's (both are set by the v_exp / v_rcp forms of sigmoid and tanh and by fp32 accumulation), and the two
    fp32 paths agree with each other far inside the stated tolerance."""
    from red_gnn_amd import engine
    torch.manual_seed(21)
    dev, n, a, ap = "cuda", 20000, 5, 8
    agg = torch.randn(n, d, device=dev) * 10.0 ** torch.empty(n, 1, device=dev).uniform_(-3, 2)
    hprev = torch.tanh(torch.randn(n // 2, d, device=dev))
    prev = torch.randint(-1, n // 2, (n,), device=dev, dtype=torch.int32)
    gate = torch.nn.GRU(d, d).to(dev)
    W_h, Ws = torch.randn(d, d, device=dev) / d ** 0.5, torch.randn(a, d, device=dev) / d ** 0.5
    f = lambda t: t.double()
    with torch.no_grad():
        x = f(agg) @ f(W_h).t()
        x = torch.relu(x) if act == "relu" else torch.tanh(x) if act == "tanh" else x
        h0 = torch.zeros(n, d, device=dev, dtype=torch.float64)
        m = prev >= 0
        h0[m] = f(hprev)[prev[m].long()]
        gi = x @ f(gate.weight_ih_l0).t() + f(gate.bias_ih_l0)
        gh = h0 @ f(gate.weight_hh_l0).t() + f(gate.bias_hh_l0)
        r, z = torch.sigmoid(gi[:, :d] + gh[:, :d]), torch.sigmoid(gi[:, d:2 * d] + gh[:, d:2 * d])
        h_ref = (1 - z) * torch.tanh(gi[:, 2 * d:] + r * gh[:, 2 * d:]) + z * h0
        as_ref = h_ref @ f(Ws).t()
        err = {}
        out = {}
        for prec in ("f16x3", "f32"):
            h, a_s = engine.dense_fwd(agg, hprev, prev, d, W_h, act, gate, Ws_next=Ws, attn_dim=a, ap=ap, precision=prec)
            err[prec] = (float((h.double() - h_ref).abs().max()), float((a_s[:, :a].double() - as_ref).abs().max()))
            out[prec] = (h, a_s)
        # (both are fp32 evaluations whose errors come from the v_exp / v_rcp forms and from fp32 rounding of pre-activations of up to
        # a few hundred: the ratio between them is noise around 1 - 0.4 .. 1.5 over these cases; a narrowed product would show as a
        # multiple)
        assert err["f16x3"][0] <= 2.0 * err["f32"][0] + 1e-7, err
        assert err["f16x3"][1] <= 2.0 * err["f32"][1] + 1e-7, err
        assert float((out["f16x3"][0] - out["f32"][0]).abs().max()) <= err["f16x3"][0] + err["f32"][0] + 1e-7, err


def test_graph_replay_inductive_switches_graphs():
    """RED_GNN_induc evaluates on two graphs of different entity counts (mode 'transductive' / 'inductive'); the replayed
    HIP graphs are keyed by the device graph and equal the eager path on both."""
    from red_gnn_amd.inductive import DataLoader as IndLoader
    from red_gnn_amd.models import RED_GNN_induc
    ids = dict(U.load("ind_WN18RR_v1_ids.npz"))
    loader = IndLoader(ids=ids, verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 3, 32, 5, loader.n_rel, "relu", 0.0

    torch.manual_seed(5)
    model = RED_GNN_induc(P, loader).cuda().eval()
    rng = np.random.default_rng(2)
    with torch.no_grad():
        for it in range(5):
            for mode, n_e in (("transductive", loader.n_ent), ("inductive", loader.n_ent_ind)):
                subs, rels = rng.integers(0, n_e, 11), rng.integers(0, 2 * loader.n_rel, 11)
                model.use_graphs = True
                s_g = model(subs, rels, mode=mode)
                model.use_graphs = False
                s_e = model(subs, rels, mode=mode)
                assert s_g.shape == (11, n_e) and torch.equal(s_g, s_e), (it, mode)
    assert len(model._graphed) == 2


def test_random_graphs_gradient_fuzz():
    """Random graphs / widths / batches: gradients of every parameter (rg_layer_bwd incl. the relation-major pass, the dA_q
    segment sums, hub rows cut into segments, sparse and dense walks) against autograd through the oracle.  tanh attention-free
    of relu kinks is not available (the attention MLP is relu by definition), so a mismatch confined to one row of a Ws/Wr/Wqr
    gradient would be a rounding flip at the kink, not a bug; none occurs with these seeds."""
    from red_gnn_amd.load_data import DataLoader
    rng = np.random.default_rng(77)
    for case in range(int(os.environ.get("RG_GRAD_FUZZ_N", "10"))):
        n_ent = int(rng.integers(20, 300))
        n_rel = int(rng.integers(1, 7))
        m = int(rng.integers(n_ent, 10 * n_ent))
        h, t = rng.integers(0, n_ent, m), rng.integers(0, n_ent, m)
        if case % 2 == 0:
            h[: m // 3] = int(rng.integers(0, n_ent))          # a hub source: its out-row is cut into segments
        facts = np.stack([h, rng.integers(0, n_rel, m), t], 1)
        ids = _ids(n_ent, n_rel, facts[: (3 * m) // 4], train=facts[(3 * m) // 4:])
        loader = DataLoader(ids=ids, verbose=False)
        d, a = int(rng.choice([16, 32, 48, 64])), int(rng.choice([3, 5, 8]))
        n_layer, act = int(rng.integers(1, 4)), str(rng.choice(["relu", "tanh", "idd"]))
        model = _random_model(loader, n_layer, d, a, act, seed=100 + case).train()
        B = int(rng.integers(1, 24))
        subs, rels = rng.integers(0, n_ent, B), rng.integers(0, 2 * n_rel, B)
        weight = torch.tensor(rng.standard_normal((B, n_ent)), dtype=torch.float32)
        s = model(subs, rels, mode="train")
        (s * weight.cuda()).sum().backward()
        p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
        ref = orc.forward(p, U.oracle_graph(ids, "train"), subs, rels, n_layer, act=act)
        np.testing.assert_allclose(s.detach().cpu().numpy(), ref.detach().numpy(), rtol=RTOL, atol=ATOL_H, err_msg="case %d" % case)
        (ref * weight).sum().backward()
        for k, v in model.named_parameters():
            r = p[k].grad.numpy() if p[k].grad is not None else np.zeros(tuple(v.shape), np.float32)
            g = v.grad.cpu().numpy() if v.grad is not None else np.zeros_like(r)
            tol = 2e-5 * max(1.0, float(np.abs(r).max()))
            bad = np.argwhere(~np.isclose(g, r, rtol=2e-3, atol=tol))
            np.testing.assert_allclose(g, r, rtol=2e-3, atol=tol, err_msg="case %d %s rows %s" % (case, k, np.unique(bad[:, 0]) if bad.size else []))


@pytest.mark.parametrize("d", [64, 128])
def test_backward_large_relation_table(d):
    """FB15k-237-like relation count (481 rows x d does not fit the LDS copy the relation-major pass normally accumulates in):
    the segments' sums go straight to global memory; forward and every gradient against autograd through the oracle."""
    from red_gnn_amd.load_data import DataLoader
    rng = np.random.default_rng(31)
    n_ent, n_rel, m = 300, 240, 5000
    facts = np.stack([rng.integers(0, n_ent, m), rng.integers(0, n_rel, m), rng.integers(0, n_ent, m)], 1)
    facts[:700, 0] = 7                                        # a hub source
    ids = _ids(n_ent, n_rel, facts[: (3 * m) // 4], train=facts[(3 * m) // 4:])
    loader = DataLoader(ids=ids, verbose=False)
    model = _random_model(loader, 2, d, 5, "tanh", seed=2).train()
    B = 9
    subs, rels = rng.integers(0, n_ent, B), rng.integers(0, 2 * n_rel, B)
    weight = torch.tensor(rng.standard_normal((B, n_ent)), dtype=torch.float32)
    s = model(subs, rels, mode="train")
    (s * weight.cuda()).sum().backward()
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    ref = orc.forward(p, U.oracle_graph(ids, "train"), subs, rels, 2, act="tanh")
    np.testing.assert_allclose(s.detach().cpu().numpy(), ref.detach().numpy(), rtol=RTOL, atol=ATOL_H)
    (ref * weight).sum().backward()
    for k, v in model.named_parameters():
        r = p[k].grad.numpy()
        np.testing.assert_allclose(v.grad.cpu().numpy(), r, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(r).max())), err_msg=k)


@pytest.mark.parametrize("act", ["relu", "tanh", "idd"])
@pytest.mark.parametrize("d,n", [(16, 37), (48, 1000), (64, 4099), (128, 300), (128, 2049), (16, 9000), (48, 20000), (64, 33000)])
def test_fused_training_dense_step_with_dropout_mask(act, d, n):
    """models._DenseStep (rg_dense_train_fwd + the manual backward) with a dropout mask, against the same step in torch ops
    (W_h, act, mask, index_copy carry, gru_cell) and autograd: output and the gradients of all seven inputs."""
    from red_gnn_amd.models import _DenseStep
    torch.manual_seed(n + d)
    dev = "cuda"
    n_old = max(1, n // 3)
    acts = {"relu": torch.relu, "tanh": torch.tanh, "idd": lambda v: v}
    gate = torch.nn.GRU(d, d).to(dev)
    leaf = lambda *shape: torch.randn(*shape, device=dev).requires_grad_(True)
    agg, hprev, W_h = leaf(n, d), leaf(n_old, d), (torch.randn(d, d, device=dev) / d ** 0.5).requires_grad_(True)
    sel = torch.randperm(n, device=dev)[:n_old]
    prev = torch.full((n,), -1, dtype=torch.int32, device=dev)
    prev[sel] = torch.arange(n_old, dtype=torch.int32, device=dev)
    old_new = sel.int()
    keep = 0.7
    mask = torch.empty(n, d, device=dev).bernoulli_(keep).div_(keep)
    w = torch.randn(n, d, device=dev)
    params = [agg, hprev, W_h, gate.weight_ih_l0, gate.weight_hh_l0, gate.bias_ih_l0, gate.bias_hh_l0]

    out = _DenseStep.apply(agg, hprev, W_h, gate.weight_ih_l0, gate.weight_hh_l0, gate.bias_ih_l0, gate.bias_hh_l0, None, prev, old_new,
                           mask, act, gate, keep)
    g1 = torch.autograd.grad((out * w).sum(), params)
    x = acts[act](agg @ W_h.t()) * mask
    h0 = torch.zeros(n, d, device=dev).index_copy(0, old_new.long(), hprev)
    ref = torch.gru_cell(x, h0, gate.weight_ih_l0, gate.weight_hh_l0, gate.bias_ih_l0, gate.bias_hh_l0)
    g2 = torch.autograd.grad((ref * w).sum(), params)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=RTOL, atol=ATOL_H)
    for a_, b_, name in zip(g1, g2, ["agg", "hidden_prev", "W_h", "w_ih", "w_hh", "b_ih", "b_hh"]):
        r = b_.cpu().numpy()
        np.testing.assert_allclose(a_.cpu().numpy(), r, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(r).max())), err_msg=name)

    # ... and with the next layer's attention projection emitted by the same kernel (rg_dense_train_fwd_as): a_s = hidden Ws^T, its
    # gradient joining the new state's (rg_rows_addmm) and Ws's own (attention widths 5 and 16)
    for attn in (5, 16):
        Ws = (torch.randn(attn, d, device=dev) / d ** 0.5).requires_grad_(True)
        ap = (attn + 3) // 4 * 4
        wa = torch.randn(n, ap, device=dev)
        out2, a_s = _DenseStep.apply(agg, hprev, W_h, gate.weight_ih_l0, gate.weight_hh_l0, gate.bias_ih_l0, gate.bias_hh_l0, Ws, prev, old_new,
                                     mask, act, gate, keep)
        assert a_s.shape == (n, ap) and torch.equal(out2, out)
        g3 = torch.autograd.grad((out2 * w).sum() + (a_s * wa).sum(), params + [Ws])
        ref2 = torch.gru_cell(acts[act](agg @ W_h.t()) * mask, torch.zeros(n, d, device=dev).index_copy(0, old_new.long(), hprev),
                              gate.weight_ih_l0, gate.weight_hh_l0, gate.bias_ih_l0, gate.bias_hh_l0)
        ref_as = ref2 @ Ws.t()
        g4 = torch.autograd.grad((ref2 * w).sum() + (ref_as * wa[:, :attn]).sum(), params + [Ws])
        np.testing.assert_allclose(a_s[:, :attn].detach().cpu().numpy(), ref_as.detach().cpu().numpy(), rtol=RTOL, atol=ATOL_H)
        assert not a_s[:, attn:].any()
        for a_, b_, name in zip(g3, g4, ["agg", "hidden_prev", "W_h", "w_ih", "w_hh", "b_ih", "b_hh", "Ws_next"]):
            r = b_.cpu().numpy()
            np.testing.assert_allclose(a_.cpu().numpy(), r, rtol=2e-3, atol=2e-5 * max(1.0, float(np.abs(r).max())), err_msg="%s attn=%d" % (name, attn))


def test_bench_plain_run_times_its_steps_and_dumps_its_outputs(tmp_path):
    """A plain bench.py run: exactly --steps timed steps, the headline fields only (no roofline, CPU baseline or family evaluation),
    and --dump-outputs writes the last step's scores, ranks and metrics, the metrics being those of the dumped ranks."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert abs(line["eval_queries_per_s"] * line["ms_per_step"] * 1e-3 - 16) < 1e-6 * 16
    for k in ("roofline", "per_hop", "roofline_dense", "dense_f32", "cpu_baseline", "parity", "family_eval"):
        assert line[k] is None, k
    scores, ranks, metrics = (np.load(str(out / (k + ".npy"))) for k in ("scores", "ranks", "metrics"))
    assert line["dumped_outputs"] == {"scores": list(scores.shape), "ranks": list(ranks.shape), "metrics": [3]}
    from red_gnn_amd.synthetic import SHAPES
    assert scores.dtype == np.float32 and scores.shape == (16, SHAPES["C2"]["n_ent"]) and np.isfinite(scores).all()
    assert ranks.dtype == np.float32 and len(ranks) >= 16 and (ranks >= 1).all() and (ranks <= scores.shape[1]).all()
    assert np.allclose(metrics, [np.mean(1.0 / ranks), np.mean(ranks <= 1), np.mean(ranks <= 10)], rtol=1e-5)
    assert abs(line["mrr_of_random_init"] - metrics[0]) < 1e-9
