"""T_RED_GNN.attention_profile on the MI355X (-m gpu): counts and alpha sums per (query | query relation, hop, direction, edge
relation) against a group-by over the float64 reference walk's edges (tests/temporal_ref.py), both bin paths of the kernel, and the
bit-for-bit properties of the integer sums.

Tolerance, as tests/test_profile_gpu.py: counts exact; |sum_dev - sum_ref| <= RTOL * sum_ref + (ATOL + Q) * count per cell."""
import numpy as np
import pytest
import torch

from tests import layer_ref as LR
from tests import temporal_ref as TR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
Q = 2.0 ** -33
AXES = ("group", "hop", "direction", "relation")


def _pad_attn(a):
    return (a + 3) // 4 * 4 if a <= 16 else 32


def lds_path(n_rela_rows, attn_dim):
    """The kernel's choice as csrc/profile.hip states it: the bins (per relation row the a_r row, 4 * ap bytes, and three 8 + 4 byte
    cells) beside the 16 KB head list in 64 KB of LDS, i.e. n_rela_rows * (4 * ap + 36) <= 49152."""
    return n_rela_rows * (4 * _pad_attn(attn_dim) + 36) <= 64 * 1024 - 4 * 2048 * 2


def _check(prof, count_ref, sum_ref, what=""):
    count, asum = prof.count.cpu().numpy(), prof.alpha_sum.cpu().numpy()
    assert prof.axes == AXES and count.shape == count_ref.shape and count.dtype == np.int64 and asum.dtype == np.float64, what
    assert np.array_equal(count, count_ref), what
    err = np.abs(asum - sum_ref)
    bound = RTOL * sum_ref + (ATOL + Q) * count_ref
    print("%s: cells with edges %d, largest |sum error| %.3g, largest error / bound %.3g"
          % (what, int((count_ref > 0).sum()), float(err.max()), float((err / np.maximum(bound, 1e-300))[count_ref > 0].max(initial=0.0))))
    assert float((err - bound).max()) <= 0.0, what
    assert (asum[count_ref == 0] == 0.0).all(), what


def _against(model, quads, n_ent, n_rows, heads, rels, times, n_layer, act, shared=False, what=""):
    _, hops, _ = TR.walk(TR.state_of(model), quads, n_ent, heads, rels, times, n_layer, act, shared_tables=shared)
    count, asum = TR.profile_cells(hops, times, len(heads), n_rows)
    batch = {"head": heads, "relation": rels, "time": times}
    pq = model.attention_profile(batch, group="query")
    assert pq.group == "query" and pq.count.is_cuda
    _check(pq, count, asum, what + " group=query")
    pr = model.attention_profile(batch)
    assert pr.group == "relation"
    _check(pr, *TR.by_relation(count, asum, rels, n_rows), what + " group=relation")
    # collapsed over direction: the per-relation table
    c = pq.collapse("direction")
    assert c.axes == ("group", "hop", "relation") and np.array_equal(c.count.cpu().numpy(), count.sum(2))
    return pq, pr, hops


@pytest.mark.parametrize("d,a,act,n_layer,shared,B", [(16, 3, "idd", 2, False, 33), (20, 5, "tanh", 3, True, 9),
                                                    (32, 30, "relu", 2, False, 1), (64, 5, "relu", 3, False, 5)])
def test_profile_vs_walk(d, a, act, n_layer, shared, B):
    c = LR._temporal_case("profile", seed=n_layer + B, B=B, m=600)
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, n_layer, d, a, act, shared=shared)
    heads, rels = c.nodes0[:, 1], (np.arange(B) * 3) % c.n_rela_rows
    assert lds_path(c.n_rela_rows, a)
    print("n_rela_rows=%d attn_dim=%d: LDS bins" % (c.n_rela_rows, a))
    pq, _, _ = _against(model, c.quads, c.n_ent, c.n_rela_rows, heads, rels, c.q_time, n_layer, act, shared, "d=%d a=%d B=%d" % (d, a, B))
    if B >= 3:                                                           # (query times 0, n_time - 1 and n_time / 2 are among them)
        assert (pq.count.sum((0, 1, 3)) > 0).all()                       # past, now and future edges all occur


def test_hand_graph_heads_of_out_degree_65_and_129():
    """Heads of out-degree 64, 65 and 129 (one flattened 64-position step, a step and one position, two steps and one), the isolated
    entity, a fact at two times around the query time; B = 6."""
    quads = TR.hand_graph()
    n_rows = 2 * TR.HAND_N_REL + 1
    model = TR.make_model(quads, TR.HAND_N_ENT, n_rows, TR.HAND_N_TIME, 2, 32, 5, "relu")
    heads, rels = np.array([0, 1, 2, 3, 299, 260]), np.array([0, 1, 2, 6, 4, 1])
    times = np.array([0, TR.HAND_N_TIME - 1, 5, 5, 3, 4])
    pq, _, _ = _against(model, quads, TR.HAND_N_ENT, n_rows, heads, rels, times, 2, "relu", what="hand")
    cnt = pq.count.cpu().numpy()
    assert cnt[:3, 0].sum((1, 2)).tolist() == [64, 65, 129] and cnt[4].sum() == 2
    # query 3 = (3, time 5), hop 1: (3, 0, 0) twice in the past (time 2, duplicated) and once in the future (time 8)
    assert cnt[3, 0, :, 0].tolist() == [2, 0, 1]


def _wide_relation_quads(n_ent, n_rel, n_time, rng, m=1500):
    h, t = rng.integers(0, n_ent - 1, m), rng.integers(0, n_ent - 1, m)
    r = rng.integers(0, n_rel, m)
    r[:4] = n_rel - 1
    tm = rng.integers(0, n_time, m)
    ent = np.arange(n_ent)
    return np.concatenate([np.column_stack([h, r, t, tm]), np.column_stack([t, r + n_rel, h, tm]),
                           np.column_stack([ent, np.full(n_ent, 2 * n_rel), ent, np.full(n_ent, n_time - 1)])], 0).astype(np.int64)


def test_both_bin_paths_give_the_walks_table():
    """901 relation rows at attn_dim 8 (901 * 68 B = 61268 > 49152: the global-atomic path) and 11 rows (the LDS path) with the same
    widths, depth and batch shape."""
    rng = np.random.default_rng(2)
    n_ent, n_time, B, d, a, n_layer = 150, 12, 5, 16, 8, 2
    for n_rel in (450, 5):
        n_rows = 2 * n_rel + 1
        quads = _wide_relation_quads(n_ent, n_rel, n_time, rng)
        path = "LDS bins" if lds_path(n_rows, a) else "global atomics"
        print("n_rela_rows=%d attn_dim=%d: %d B of bins against 49152 -> %s" % (n_rows, a, n_rows * (4 * _pad_attn(a) + 36), path))
        assert lds_path(n_rows, a) == (n_rel == 5) and (n_rel == 5 or n_rows >= 900)
        model = TR.make_model(quads, n_ent, n_rows, n_time, n_layer, d, a, "relu")
        heads = rng.integers(0, n_ent, B)
        heads[0] = n_ent - 1                                             # identity edge only
        rels = np.array([0, n_rows - 1, n_rel, 1, n_rel + 1])
        times = np.array([0, n_time - 1, 5, 3, 7])
        _against(model, quads, n_ent, n_rows, heads, rels, times, n_layer, "relu", what=path)


def test_integer_sums_split_permutation_and_explain():
    c = LR._temporal_case("bits", seed=8, B=33, m=600)
    n_layer, a = 2, 5
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, n_layer, 32, a, "relu")
    heads, rels, times = c.nodes0[:, 1], (np.arange(33) * 3) % c.n_rela_rows, c.q_time
    sub = lambda idx: {"head": heads[idx], "relation": rels[idx], "time": times[idx]}
    same = lambda p, q: torch.equal(p.count, q.count) and torch.equal(p.fixed, q.fixed)
    every = np.arange(33)
    whole = model.attention_profile(sub(every))
    assert same(whole, model.attention_profile(sub(every)))              # two runs
    for cuts in ([1], [16], [5, 6, 20], list(range(1, 33))):
        parts = np.split(every, cuts)
        acc = None
        for part in parts:
            p = model.attention_profile(sub(part))
            acc = p if acc is None else acc + p
        assert same(whole, acc), cuts
    perm = np.random.default_rng(0).permutation(33)
    assert same(whole, model.attention_profile(sub(perm)))
    pq = model.attention_profile(sub(every), group="query")
    pp = model.attention_profile(sub(perm), group="query")
    assert torch.equal(pq.count[perm], pp.count) and torch.equal(pq.fixed[perm], pp.fixed)
    # explain with one row per last-level entity of a query: its hop-L edges are all hop-L edges of the query, so their alphas,
    # rounded and summed in int64 on the host by (direction, relation), are the profile's hop-L cells
    for q in (0, 1, 7):
        with torch.no_grad():
            model(sub(np.array([q])), mode="test")
        last = model.last_nodes.cpu().numpy()[:, 1]
        rows = np.full(len(last), q)
        rd = model.explain(sub(rows), last)
        assert rd.reached.all()
        e, al, dr = rd.edges.cpu().numpy(), rd.alpha.cpu().numpy(), rd.direction().cpu().numpy().astype(np.int64)
        m = e[:, 1] == n_layer
        fx = np.rint(al[m].astype(np.float32) * np.float32(4294967296.0)).astype(np.int64)      # llrintf(alpha * 2^32), exact in fp32
        fixed = np.zeros((3, c.n_rela_rows), np.int64)
        count = np.zeros((3, c.n_rela_rows), np.int64)
        np.add.at(fixed, (dr[m], e[m, 3]), fx)
        np.add.at(count, (dr[m], e[m, 3]), 1)
        assert np.array_equal(count, pq.count[q, n_layer - 1].cpu().numpy()), q
        assert np.array_equal(fixed, pq.fixed[q, n_layer - 1].cpu().numpy()), q


def test_arguments_are_validated():
    from red_gnn_amd import _lib, engine
    quads = TR.hand_graph()
    n_ent, R = TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1
    model = TR.make_model(quads, n_ent, R, TR.HAND_N_TIME, 2, 16, 3, "idd")
    ok = {"head": [0], "relation": [0], "time": [0]}
    for bad in ({"head": [n_ent]}, {"relation": [R]}, {"time": [TR.HAND_N_TIME]}, {"time": [-1]}, {"relation": [0, 1]}):
        with pytest.raises(ValueError):
            model.attention_profile({**ok, **bad})
    with pytest.raises(ValueError):
        model.attention_profile(ok, group="time")
    # the entry point: static graph, windowed frontier, NULL q_time
    L, s = _lib.lib(), _lib.stream_ptr()
    sg = engine.Graph(n_ent, TR.HAND_N_REL, quads[:100, :3])
    out = torch.zeros((4, 3, R), dtype=torch.int64, device="cuda")
    f32 = torch.zeros((R, 4), dtype=torch.float32, device="cuda")
    qt = torch.zeros(4, dtype=torch.int32, device="cuda")

    def frontier(graph, window=False):
        fr = engine.Frontier(n_ent, 4, 3)
        fr.reset(torch.zeros(4, dtype=torch.int32, device="cuda"))
        fr.expand(graph)
        if window:
            fr.set_window(qt, qt + 5, 10)
        return fr

    def call(fr, g, q_time=qt, n_old=4):
        return L.rg_tattn_profile(fr.handle, g.handle, 4, n_ent, 1, n_old, _lib.ptr(q_time), _lib.ptr(f32), _lib.ptr(f32), _lib.ptr(f32),
                                  4, _lib.ptr(f32), _lib.ptr(f32), 3, _lib.ptr(out), _lib.ptr(out), s)
    assert call(frontier(sg), sg) != 0 and b"temporal graphs only" in L.rg_last_error()
    assert call(frontier(model.graph, True), model.graph) != 0 and b"window" in L.rg_last_error()
    assert call(frontier(model.graph), model.graph, q_time=None) != 0 and b"NULL" in L.rg_last_error()
    assert call(frontier(model.graph), model.graph, n_old=5) != 0 and b"n_old" in L.rg_last_error()
    torch.cuda.synchronize()
    assert (out == 0).all()
