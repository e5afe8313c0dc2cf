"""RDigraph.top_paths (rg_paths_topk, csrc/paths.hip) on the MI355X (-m gpu) against tests/paths_ref.py on hand-built digraphs: edge
indices and counts exactly, products bit for bit - every product is the same chain of IEEE float64 multiplications."""
import numpy as np
import pytest
import torch

from tests import paths_ref as R

pytestmark = pytest.mark.gpu

KS = (1, 3, 8)


def _rd(edges, alpha, offsets, L, **kw):
    from red_gnn_amd.explain import RDigraph
    B = len(offsets) - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return RDigraph(edges=dev(edges.astype(np.int32).reshape(-1, 5)), alpha=dev(alpha.astype(np.float32)),
                    offsets=dev(np.asarray(offsets, dtype=np.int64)), reached=torch.ones(B, dtype=torch.bool, device="cuda"),
                    score=torch.zeros(B, device="cuda"), n_hops=L, **{k: dev(v) for k, v in kw.items()})


def _check(ps, ref, what=""):
    edge, prod, count = ref
    assert ps.edge.dtype == torch.int64 and ps.product.dtype == torch.float64 and ps.count.dtype == torch.int32
    assert np.array_equal(ps.count.cpu().numpy(), count), what
    assert np.array_equal(ps.edge.cpu().numpy(), edge), what
    assert ps.product.cpu().numpy().tobytes() == prod.tobytes(), what


def test_random_digraphs_without_ties():
    rng = np.random.default_rng(7)
    edges, alpha, offsets = R.layered_digraph(rng, B=6, L=3, n_ent=200, width=12, rels_per_pair=3, p_edge=1.0, n_rel=6, min_rels=2)
    _, prod9, count9 = R.dp(edges, alpha, offsets, 3, 9)
    assert (count9 == 9).all() and (np.diff(prod9, axis=1) < 0).all()        # no product tie among each row's first k + 1 paths
    rd = _rd(edges, alpha, offsets, 3)
    for k in KS:
        _check(rd.top_paths(k), R.dp(edges, alpha, offsets, 3, k), k)


def test_ties_follow_the_recursive_order():
    rng = np.random.default_rng(3)
    edges, alpha, offsets = R.layered_digraph(rng, B=4, L=3, n_ent=30, width=4, rels_per_pair=2, p_edge=0.8, alphas=(0.5,), n_rel=3,
                                              dangling=2)
    rd = _rd(edges, alpha, offsets, 3)
    for k in KS:
        ref = R.brute_force(edges, alpha, offsets, 3, k)
        assert (ref[2] == k).all() and (ref[1] == 0.125).all()               # every kept path ties with every other
        _check(rd.top_paths(k), ref, k)


def _edge_rows():
    """L = 3.  Row 0: empty.  Row 1: hops 1 and 2 only.  Row 2: two paths.  Row 3: dangling heads at hops 2 and 3, one of them the
    edge of the largest alpha.  Row 4: hop 3 present but reached by nothing."""
    rows = [
        [],
        [(1, 0, 0, 1), (1, 0, 1, 2), (2, 1, 0, 3), (2, 2, 0, 3)],
        [(1, 0, 0, 1), (2, 1, 0, 2), (2, 1, 1, 2), (3, 2, 0, 9)],
        [(1, 0, 0, 1), (1, 0, 0, 2), (2, 1, 0, 4), (2, 7, 0, 4), (2, 2, 1, 5), (3, 4, 0, 9), (3, 5, 0, 9), (3, 6, 0, 9)],
        [(1, 0, 0, 1), (2, 1, 0, 2), (3, 5, 0, 9)],
    ]
    alphas = [[], [0.5] * 4, [0.5, 0.25, 0.75, 0.5], [0.5, 0.25, 0.5, 0.99, 0.5, 0.5, 0.5, 1.0], [0.5] * 3]
    edges = np.array([(b,) + e for b, es in enumerate(rows) for e in es], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(es) for es in rows])])
    return edges, np.array([a for al in alphas for a in al], dtype=np.float32), offsets


def test_edge_rows():
    edges, alpha, offsets = _edge_rows()
    rd = _rd(edges, alpha, offsets, 3)
    for k in KS:
        ref = R.brute_force(edges, alpha, offsets, 3, k)
        assert ref[2].tolist() == [0, 0, min(k, 2), min(k, 2), 0]
        ps = rd.top_paths(k)
        _check(ps, ref, k)
        assert (ps.rels()[0] == -1).all() and (ps.entities()[4] == -1).all()
    assert rd.top_paths(8).rels()[2, :2].tolist() == [[0, 1, 0], [0, 0, 0]]      # 0.5 * 0.75 * 0.5 before 0.5 * 0.25 * 0.5


@pytest.mark.parametrize("L", [1, 5])
def test_shortest_and_longest(L):
    rng = np.random.default_rng(L)
    edges, alpha, offsets = R.layered_digraph(rng, B=3, L=L, n_ent=50, width=3, rels_per_pair=3, p_edge=0.8, alphas=(0.25, 0.5, 1.0),
                                              n_rel=4, dangling=1)
    rd = _rd(edges, alpha, offsets, L)
    for k in KS:
        ref = R.brute_force(edges, alpha, offsets, L, k)
        assert (ref[2] > 0).all()
        _check(rd.top_paths(k), ref, (L, k))


def test_hub_group_and_many_groups():
    """Row 1 of 2: hop 1 has 600 groups (the scan crosses tiles of the 256-thread workgroup), hop 3 is one group of 300 in-edges from
    40 heads (lanes hold several candidates each and the wave merge runs)."""
    rng = np.random.default_rng(5)
    mids, heads = np.arange(100, 700), np.arange(1000, 1040)
    rows = [(1, 0, int(rng.integers(4)), int(m)) for m in mids]
    for m in mids:
        for h in rng.choice(heads, int(rng.integers(1, 3)), replace=False):
            rows.append((2, int(m), int(rng.integers(4)), int(h)))
    pairs = rng.permutation(40 * 10)[:300]
    rows += [(3, int(heads[p // 10]), int(p % 10), 5000) for p in pairs]
    e = np.array(rows, dtype=np.int64)
    e = e[rng.permutation(len(e))]
    e = e[np.lexsort((e[:, 3], e[:, 0]))]
    assert len(np.unique(e[e[:, 0] == 1, 3])) == 600 and (e[:, 0] == 3).sum() == 300 and len(np.unique(e[e[:, 0] == 3, 1])) == 40
    small, small_a, _ = R.layered_digraph(rng, B=1, L=3, n_ent=20, width=3, rels_per_pair=2, p_edge=1.0)
    edges = np.concatenate([small, np.concatenate([np.ones((len(e), 1), dtype=np.int64), e], 1).astype(np.int32)], 0)
    alpha = np.concatenate([small_a, rng.uniform(0.05, 1.0, len(e)).astype(np.float32)])
    offsets = np.array([0, len(small), len(edges)])
    rd = _rd(edges, alpha, offsets, 3)
    for k in KS:
        ref = R.dp(edges, alpha, offsets, 3, k)
        assert (ref[2] == k).all()
        _check(rd.top_paths(k), ref, k)


def test_rows_are_independent():
    from red_gnn_amd import engine
    rng = np.random.default_rng(9)
    edges, alpha, offsets = R.layered_digraph(rng, B=7, L=3, n_ent=60, width=6, rels_per_pair=2, p_edge=0.7, alphas=(0.25, 0.5, 1.0),
                                              n_rel=4, dangling=1)
    rd = _rd(edges, alpha, offsets, 3)
    lo, hi = int(offsets[2]), int(offsets[5])
    part = _rd(edges[lo:hi], alpha[lo:hi], offsets[2:6] - lo, 3)
    for k in KS:
        whole, alone = rd.top_paths(k), part.top_paths(k)
        _check(whole, R.dp(edges, alpha, offsets, 3, k), k)
        shifted = torch.where(alone.edge >= 0, alone.edge + lo, alone.edge)
        assert torch.equal(whole.edge[2:5], shifted) and torch.equal(whole.count[2:5], alone.count)
        assert whole.product[2:5].cpu().numpy().tobytes() == alone.product.cpu().numpy().tobytes()
        assert engine.paths_scratch_bytes(1, k) > 1
        single = rd.top_paths(k, scratch_bytes=1)                              # every row is its own chunk
        assert torch.equal(single.edge, whole.edge) and torch.equal(single.count, whole.count)
        assert single.product.cpu().numpy().tobytes() == whole.product.cpu().numpy().tobytes()


def test_times_and_data_rows():
    edges, alpha, offsets = _edge_rows()
    time = (np.arange(len(edges)) * 3 + 1).astype(np.int32)
    rows = (np.arange(len(edges)) + 100).astype(np.int32)
    rd = _rd(edges, alpha, offsets, 3, time=time, q_time=np.zeros(5, dtype=np.int32), data_row=rows)
    ps = rd.top_paths(3)
    edge = ps.edge.cpu().numpy()
    for got, col in ((ps.times(), time), (ps.data_rows(), rows)):
        assert np.array_equal(got.cpu().numpy(), np.where(edge >= 0, col[np.clip(edge, 0, None)], -1))
    assert ps.times()[2, 0].tolist() == [int(time[offsets[2]]), int(time[offsets[2] + 2]), int(time[offsets[2] + 3])]
    with pytest.raises(ValueError):
        _rd(edges, alpha, offsets, 3).top_paths(2).times()
    with pytest.raises(ValueError):
        _rd(edges, alpha, offsets, 3).top_paths(2).data_rows()
