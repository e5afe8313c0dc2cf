"""The host references of top_paths against each other and against RDigraph.strongest_paths (no GPU): the k-truncated dynamic
programme loses nothing against full enumeration under the recursive order, ties everywhere."""
import numpy as np
import pytest
import torch

from tests import paths_ref as R


def _cases(n, seed):
    rng = np.random.default_rng(seed)
    for i in range(n):
        L = 1 + i % 4
        B = int(rng.integers(1, 4))
        yield L, R.layered_digraph(rng, B, L, n_ent=8, width=int(rng.integers(1, 4)), rels_per_pair=2, p_edge=0.7,
                                   alphas=(0.25, 0.5, 1.0), n_rel=3, dangling=int(rng.integers(0, 3)))


def _same(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y)) and x[1].tobytes() == y[1].tobytes()


def test_dp_equals_brute_force_with_ties():
    n_ties = n_short = 0
    for L, (edges, alpha, offsets) in _cases(200, seed=11):
        for k in (1, 2, 8):
            bf, dp = R.brute_force(edges, alpha, offsets, L, k), R.dp(edges, alpha, offsets, L, k)
            assert _same(bf, dp), (L, k)
            assert (dp[2] <= k).all() and ((dp[0][..., 0] >= 0).sum(1) == dp[2]).all()
        prod, count = bf[1], bf[2]
        n_ties += int(((prod[:, 1:] == prod[:, :-1]) & (np.arange(1, 8)[None] < count[:, None])).sum())
        n_short += int(((count > 0) & (count < 8)).sum())
    assert n_ties > 100 and n_short > 10         # the cases do hold product ties and rows with fewer than k paths


def test_paths_are_paths_in_order():
    for L, (edges, alpha, offsets) in _cases(40, seed=5):
        edge, prod, count = R.dp(edges, alpha, offsets, L, 8)
        for b in range(len(count)):
            for i in range(count[b]):
                es = edge[b, i]
                assert (offsets[b] <= es).all() and (es < offsets[b + 1]).all()
                assert (edges[es, 1] == np.arange(1, L + 1)).all() and (edges[es[1:], 2] == edges[es[:-1], 4]).all()
                p = np.float64(1.0)
                for x in es:
                    p = p * np.float64(alpha[x])
                assert p == prod[b, i]
            assert (np.diff(prod[b, :count[b]]) <= 0).all()
            assert len({tuple(x) for x in edge[b, :count[b]]}) == count[b]


def test_brute_force_k1_is_strongest_paths():
    from red_gnn_amd.explain import RDigraph
    for L, (edges, alpha, offsets) in _cases(100, seed=23):
        B = len(offsets) - 1
        rd = RDigraph(edges=torch.from_numpy(edges), alpha=torch.from_numpy(alpha), offsets=torch.from_numpy(offsets),
                      reached=torch.ones(B, dtype=torch.bool), score=torch.zeros(B), n_hops=L)
        rels, ents, prod = (t.numpy() for t in rd.strongest_paths())
        edge, p1, count = R.brute_force(edges, alpha, offsets, L, 1)
        have = count > 0
        es = edge[have, 0]
        assert np.array_equal(rels[have], edges[es, 3]) and (rels[~have] == -1).all()
        assert np.array_equal(ents[have], np.concatenate([edges[es, 2], edges[es[:, -1:], 4]], 1)) and (ents[~have] == -1).all()
        assert prod.tobytes() == p1[:, 0].tobytes()


def test_rows_without_paths():
    # row 0: no edges; row 1: hops 1..2 of 3 only; row 2: a hop-3 edge whose head no hop-2 edge reaches
    edges = np.array([[1, 1, 0, 0, 1], [1, 2, 1, 0, 2],
                      [2, 1, 0, 0, 1], [2, 2, 1, 0, 2], [2, 3, 7, 0, 3]], dtype=np.int32)
    alpha = np.full(5, 0.5, dtype=np.float32)
    offsets = np.array([0, 0, 2, 5])
    for f in (R.brute_force, R.dp):
        edge, prod, count = f(edges, alpha, offsets, 3, 2)
        assert (count == 0).all() and (edge == -1).all() and (prod == 0).all()
