"""numpy restatement of the r-digraph definition (RED_GNN_trans.explain) for the explain tests: backward marks from o, the alpha
threshold, one forward sweep from s, and the stated output order."""
import numpy as np


def rdigraph_mask(row, hop, head, tail, alpha, objs, reached, tau, n_ent, L):
    """Which edges of a hop-labelled subgraph edge list belong to the r-digraphs of rows (s, r, objs[row]) at threshold tau."""
    row, hop, head, tail = (np.asarray(x, dtype=np.int64) for x in (row, hop, head, tail))
    alpha = np.asarray(alpha)
    ok = np.zeros(len(row), dtype=bool)
    b_r = np.nonzero(np.asarray(reached))[0]
    marks = np.unique(b_r * n_ent + np.asarray(objs, dtype=np.int64)[b_r])
    for l in range(L, 0, -1):
        m = (hop == l) & (alpha >= tau) & np.isin(row * n_ent + tail, marks)
        ok |= m
        marks = np.unique(row[m] * n_ent + head[m])
    for l in range(2, L + 1):
        reach = np.unique(row[ok & (hop == l - 1)] * n_ent + tail[ok & (hop == l - 1)])
        h = hop == l
        ok[h] &= np.isin(row[h] * n_ent + head[h], reach)
    return ok


def csr_positions(graph, heads, rels, tails):
    """Position of each (head, rel) -> tail edge in the device graph's CSR by tail (first one for duplicated facts)."""
    _, _, ip, ihr = graph.export()
    pos = {}
    for t in np.unique(np.asarray(tails)):
        for q in range(ip[t], ip[t + 1]):
            pos.setdefault((int(t), int(ihr[q, 0]), int(ihr[q, 1])), q)
    return np.array([pos[(int(t), int(h), int(r))] for h, r, t in zip(heads, rels, tails)], dtype=np.int64)


def expected_digraph(hop_edges, hop_alpha, objs, last_nodes, tau, n_ent, graph):
    """r-digraphs of rows (b, objs[b]) from the subgraph edges of every hop.  hop_edges[l-1]: [E_l, >=4] = (query, head, rel, tail, ...)
    of hop l for the batch's queries; the rows here are queries (one row per query).  Returns (edges [E,5], alpha [E], offsets [B+1],
    reached [B]) in the stated order."""
    L = len(hop_edges)
    B = len(objs)
    last = set(map(tuple, np.asarray(last_nodes)[:, :2].tolist()))
    reached = np.array([(b, int(objs[b])) in last for b in range(B)])
    cat = np.concatenate([np.concatenate([np.asarray(e)[:, :4].astype(np.int64), np.full((len(e), 1), l + 1)], 1)
                          for l, e in enumerate(hop_edges)], 0)
    al = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a in hop_alpha])
    row, head, rel, tail, hop = cat.T
    ok = rdigraph_mask(row, hop, head, tail, al, objs, reached, tau, n_ent, L)
    row, head, rel, tail, hop, al = row[ok], head[ok], rel[ok], tail[ok], hop[ok], al[ok]
    pos = csr_positions(graph, head, rel, tail) if len(row) else np.zeros(0, np.int64)
    o = np.lexsort((pos, tail, hop, row))
    edges = np.stack([row, hop, head, rel, tail], 1)[o]
    offsets = np.zeros(B + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(edges[:, 0], minlength=B)) if len(edges) else 0
    return edges, al[o], offsets, reached


def expand_rows(hop_edges, query_of_row):
    """Subgraph edges per hop for rows that repeat queries: row i uses query query_of_row[i]'s edges."""
    out = []
    for e in hop_edges:
        e = np.asarray(e)
        parts = []
        for i, q in enumerate(query_of_row):
            sel = e[e[:, 0] == q]
            parts.append(np.concatenate([np.full((len(sel), 1), i), sel[:, 1:4]], 1))
        out.append(np.concatenate(parts, 0) if parts else np.zeros((0, 4), np.int64))
    return out


def expand_alpha(hop_edges, hop_alpha, query_of_row):
    out = []
    for e, a in zip(hop_edges, hop_alpha):
        e, a = np.asarray(e), np.asarray(a).reshape(-1)
        out.append(np.concatenate([a[e[:, 0] == q] for q in query_of_row]) if len(query_of_row) else np.zeros(0))
    return out
