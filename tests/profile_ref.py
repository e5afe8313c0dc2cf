"""numpy reference of the attention profile: a group-by over per-hop edge lists.

hop_edges[l]: int array [E_l, >= 4] whose first four columns are (query, head, rel, tail) - the layout of the reference's
sampled_edges, of the oracle's trace and of RDigraph rows without their hop column; hop_alpha[l]: float64 [E_l].
"""
import numpy as np


def profile_by_query(hop_edges, hop_alpha, n_query, n_rows):
    """(count int64 [B, L, n_rows], alpha_sum float64 [B, L, n_rows]): per query, hop and edge relation the number of edges and the
    sum of alpha (float64 adds in edge-list order)."""
    L = len(hop_edges)
    count = np.zeros((n_query, L, n_rows), np.int64)
    asum = np.zeros((n_query, L, n_rows), np.float64)
    for l, (e, a) in enumerate(zip(hop_edges, hop_alpha)):
        e = np.asarray(e).astype(np.int64)
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        assert len(e) == len(a)
        np.add.at(count[:, l], (e[:, 0], e[:, 2]), 1)
        np.add.at(asum[:, l], (e[:, 0], e[:, 2]), a)
    return count, asum


def by_relation(count, asum, rels, n_rows):
    """The per-query tables summed over the rows with the same query relation: [n_rows, L, n_rows] each."""
    rels = np.asarray(rels).astype(np.int64)
    c = np.zeros((n_rows,) + count.shape[1:], np.int64)
    s = np.zeros((n_rows,) + asum.shape[1:], np.float64)
    np.add.at(c, rels, count)
    np.add.at(s, rels, asum)
    return c, s
