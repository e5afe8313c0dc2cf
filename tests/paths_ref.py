"""Host references of RDigraph.top_paths (rg_paths_topk) on a compact edge list, in numpy:

    brute_force  a DFS that enumerates every path of a row and sorts them with the recursive comparator of the definition;
    dp           the k-truncated dynamic programme over (level, node), the algorithm the kernel runs.

Both take edges int [E, 5] = (row, hop, head, rel, tail) ordered by (row, hop, tail, position), alpha float32 [E], offsets [B + 1],
the hop count L and k, and return (edge int64 [B, k, L] (-1 past the count), product float64 [B, k] (0 past it), count int32 [B]).
A path is L edges e_1..e_L of the row with hop(e_l) = l, tail(e_l) = head(e_l+1) and e_L in the run of (hop, tail) that ends the row,
which must be a hop-L run; its product is ((1.0 * a_1) * a_2) ... * a_L in float64.  P comes before Q at level l if P's product is
larger, else if P's last edge has the smaller (head, rel, edge index), else (same last edge) if P's prefix comes first at level l - 1.
"""
import functools

import numpy as np


def _last_group(e, lo, hi, L):
    """Edge indices of the run of (hop, tail) that ends the row's edges [lo, hi), if it is a hop-L run (else none)."""
    if hi <= lo or e[hi - 1, 1] != L:
        return range(0)
    g = hi - 1
    while g > lo and e[g - 1, 1] == L and e[g - 1, 4] == e[hi - 1, 4]:
        g -= 1
    return range(g, hi)


def _pack(paths, k, L):
    """paths: per row the sorted list of (edge tuple, product)."""
    B = len(paths)
    edge = np.full((B, k, L), -1, dtype=np.int64)
    prod = np.zeros((B, k), dtype=np.float64)
    count = np.zeros(B, dtype=np.int32)
    for b, rows in enumerate(paths):
        count[b] = min(k, len(rows))
        for i, (es, p) in enumerate(rows[:k]):
            edge[b, i] = es
            prod[b, i] = p
    return edge, prod, count


def brute_force(edges, alpha, offsets, L, k):
    e = np.asarray(edges).astype(np.int64).reshape(-1, 5)
    a = np.asarray(alpha, dtype=np.float32)
    out = []
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        by_head = [dict() for _ in range(L + 2)]                    # by_head[l][head] = hop-l edges of the row with that head
        for i in range(lo, hi):
            if 1 <= e[i, 1] <= L:
                by_head[e[i, 1]].setdefault(int(e[i, 2]), []).append(i)
        last = set(_last_group(e, lo, hi, L))
        found = []                                                  # (edges, prefix products p_1..p_L)

        def walk(es, ps):
            l = len(es)
            if l == L:
                if es[-1] in last:
                    found.append((tuple(es), tuple(ps)))
                return
            for i in by_head[l + 1].get(int(e[es[-1], 4]), []):
                walk(es + [i], ps + [ps[-1] * np.float64(a[i])])

        for i in range(lo, hi):
            if e[i, 1] == 1:
                walk([i], [np.float64(1.0) * np.float64(a[i])])

        def cmp(P, Q, l=L):
            (pe, pp), (qe, qp) = P, Q
            if pp[l - 1] != qp[l - 1]:
                return -1 if pp[l - 1] > qp[l - 1] else 1
            kp, kq = (e[pe[l - 1], 2], e[pe[l - 1], 3], pe[l - 1]), (e[qe[l - 1], 2], e[qe[l - 1], 3], qe[l - 1])
            if kp != kq:
                return -1 if kp < kq else 1
            return cmp(P, Q, l - 1) if l > 1 else 0

        found.sort(key=functools.cmp_to_key(cmp))
        out.append([(es, ps[-1]) for es, ps in found])
    return _pack(out, k, L)


def dp(edges, alpha, offsets, L, k):
    e = np.asarray(edges).astype(np.int64).reshape(-1, 5)
    a = np.asarray(alpha, dtype=np.float32)
    out = []
    for b in range(len(offsets) - 1):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        prev, rows = None, []                    # prev[node] = the node's <= k best prefixes (product, edges), best first
        hop = e[lo:hi, 1]
        for l in range(1, L + 1):
            cand = {}                            # tail -> [(-product, head, rel, edge, prefix rank, edges)]
            for i in (lo + np.nonzero(hop == l)[0]).tolist():
                pre = [(np.float64(1.0), ())] if l == 1 else prev.get(int(e[i, 2]), [])
                for j, (p, es) in enumerate(pre):
                    cand.setdefault(int(e[i, 4]), []).append((-(p * np.float64(a[i])), int(e[i, 2]), int(e[i, 3]), i, j, es + (i,)))
            prev = {t: [(-c[0], c[5]) for c in sorted(cs, key=lambda c: c[:5])[:k]] for t, cs in cand.items()}
        last = _last_group(e, lo, hi, L)
        if len(last):
            rows = [(es, p) for p, es in prev.get(int(e[last[0], 4]), [])]
        out.append(rows)
    return _pack(out, k, L)


def layered_digraph(rng, B, L, n_ent, width, rels_per_pair, p_edge, alphas=None, n_rel=5, dangling=0, min_rels=1):
    """A random batch of layered digraphs in the compact layout.  Row b: level 0 = {s}, levels 1..L-1 = ``width`` random entities each,
    level L = {o}; every (node of level l-1, node of level l) pair is joined with probability ``p_edge`` by ``min_rels``..``rels_per_pair``
    relations; ``dangling`` more edges per hop >= 2 leave entities outside the level before.  Edges of a (hop, tail) run are in random
    order.  alpha: drawn from ``alphas`` if given (ties), else random float32 in (0, 1).
    Returns (edges int32 [E, 5], alpha float32 [E], offsets int64 [B + 1])."""
    all_e, offsets = [], [0]
    for b in range(B):
        levels = [rng.choice(n_ent, 1)] + [rng.choice(n_ent, min(width, n_ent), replace=False) for _ in range(L - 1)] + [rng.choice(n_ent, 1)]
        rows = []
        for l in range(1, L + 1):
            for h in levels[l - 1]:
                for t in levels[l]:
                    if l == 1 or l == L or rng.random() < p_edge:
                        for r in rng.choice(n_rel, rng.integers(min_rels, rels_per_pair + 1), replace=False):
                            rows.append((b, l, int(h), int(r), int(t)))
            for _ in range(dangling if l >= 2 else 0):
                h = int(rng.integers(n_ent, 2 * n_ent))            # an entity id no level holds
                rows.append((b, l, h, int(rng.integers(n_rel)), int(rng.choice(levels[l]))))
        rows = np.array(rows, dtype=np.int64).reshape(-1, 5)
        rows = rows[rng.permutation(len(rows))]
        rows = rows[np.lexsort((rows[:, 4], rows[:, 1]))]          # stable: (hop, tail), random order inside a run
        all_e.append(rows)
        offsets.append(offsets[-1] + len(rows))
    edges = np.concatenate(all_e, 0).astype(np.int32)
    if alphas is None:
        alpha = rng.uniform(0.05, 1.0, len(edges)).astype(np.float32)
    else:
        alpha = rng.choice(np.asarray(alphas, dtype=np.float32), len(edges))
    return edges, alpha, np.array(offsets, dtype=np.int64)
