"""Dense set-expansion reference of the frontier (what include/redgnn.h promises for rg_frontier_reset / reset_nodes / expand* /
nodes / edges / level_counts), in plain numpy, plus the case table the frontier tests share.  TEST INFRASTRUCTURE.

Deliberately another method than the kernels (bit-parallel words, popcount ranks) and than oracle.get_neighbors (CSR by head, two
np.unique sorts); neither is imported here.

    edge list   static (rg_graph_create): the triples, then their inverses (t, r + n_rel, h), then one identity row (e, 2 n_rel, e) per
                entity - fact-row order.  Temporal (rg_tgraph_create): the quadruples as given; ``row`` is their time field.
    level       a boolean matrix cur[B, n_ent]
    hop         valid[b, e] = cur[b, head[e]] & in_window(b, e)
                in_window = True without windows, else  row[e] >= n_data  or  win_lo[b] <= row[e] < win_hi[b]
                new[b, t] = any valid edge into t;   E = valid.sum()
    node list   np.argwhere(new): (b, entity) order;  prev_idx = rank in the old level or -1;  old_nodes_new_idx = rank of every old
                node in the new level
    edges       [E, 6] = (b, head, rel, tail, old_idx, new_idx) grouped by new_idx and, inside a destination, in the order the
                CSR-by-tail lists the edges: a stable sort of the fact rows by tail (Graph.export()'s in_head_rel)
    row_ptr     [N_new + 1]: the segment of every destination in ``edges``
"""
import functools
import types

import numpy as np

SMALL_FUSED_WORDS = 1024       # frontier.hip enqueue_expand: `split_emit = (nodes || prev_idx) && nw > 1024`
SMALL_MAX_WORDS = 12288        # frontier.hip: `if (nw <= SMALL_MAX_WORDS)` - one workgroup, else transpose + scan + pack
VROW_MAX = 128                 # common.h RG_VROW_MAX: in-edges per virtual row of the CSR-by-tail


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def edge_list(case):
    """(head, rel, tail, row) of every fact row, in fact-row order; row is None for a static graph."""
    if case.kind == "static":
        t = np.asarray(case.triples, np.int64).reshape(-1, 3)
        ent = np.arange(case.n_ent, dtype=np.int64)
        return types.SimpleNamespace(head=np.concatenate([t[:, 0], t[:, 2], ent]),
                                     rel=np.concatenate([t[:, 1], t[:, 1] + case.n_rel, np.full(case.n_ent, 2 * case.n_rel)]),
                                     tail=np.concatenate([t[:, 2], t[:, 0], ent]), row=None)
    q = np.asarray(case.quads, np.int64).reshape(-1, 4)
    return types.SimpleNamespace(head=q[:, 0], rel=q[:, 1], tail=q[:, 2], row=q[:, 3])


def level0(case):
    cur = np.zeros((case.B, case.n_ent), dtype=bool)
    cur[case.nodes0[:, 0], case.nodes0[:, 1]] = True
    return cur


def _ranks(level):
    r = np.full(level.shape, -1, dtype=np.int64)
    r[level] = np.arange(int(level.sum()))
    return r


def hop(case, el, cur, windows=None):
    """One hop from the level ``cur``.  windows: follow the case's row windows (default: the case is of kind "windowed")."""
    windows = case.kind == "windowed" if windows is None else windows
    B, n_ent = cur.shape
    valid = cur[:, el.head]
    if windows:
        r = el.row[None, :]
        valid = valid & ((r >= case.n_data) | ((r >= case.win_lo[:, None]) & (r < case.win_hi[:, None])))
    order = np.argsort(el.tail, kind="stable")                     # the CSR-by-tail: fact-row order inside a tail
    ptr = np.concatenate([[0], np.cumsum(np.bincount(el.tail, minlength=n_ent))])
    vs = valid[:, order]
    c = np.zeros((B, len(order) + 1), dtype=np.int64)
    np.cumsum(vs, axis=1, out=c[:, 1:])
    deg = c[:, ptr[1:]] - c[:, ptr[:-1]]                           # valid in-edges of (b, t)
    new = deg > 0
    rank_old, rank_new = _ranks(cur), _ranks(new)
    bb, ee = np.nonzero(vs)                                        # by b, then tail, then CSR position: grouped by new_idx
    h, rl, t = el.head[order][ee], el.rel[order][ee], el.tail[order][ee]
    edges = np.stack([bb, h, rl, t, rank_old[bb, h], rank_new[bb, t]], 1)
    return types.SimpleNamespace(cur=new, nodes=np.argwhere(new), prev_idx=rank_old[new], old_new=rank_new[cur], n_old=int(cur.sum()),
                                 n_new=int(new.sum()), E=int(valid.sum()), edges=edges,
                                 row_ptr=np.concatenate([[0], np.cumsum(deg[new])]))


def run(case, windows=None, n_hops=None):
    """[hop 1, hop 2, ...] of the case from its level 0."""
    el, cur, out = edge_list(case), level0(case), []
    for _ in range(case.hops if n_hops is None else n_hops):
        out.append(hop(case, el, cur, windows))
        cur = out[-1].cur
    return out


@functools.lru_cache(maxsize=None)
def case_and_ref(name):
    """(case, its hops) computed once per process; callers must not modify either."""
    case = CASES[name]()
    return case, run(case)


def counts(case, hops):
    """What rg_frontier_level_counts lists after these hops: [(N_l, E_l)], level 0 first (its E is 0)."""
    return [(len(case.nodes0), 0)] + [(h.n_new, h.E) for h in hops]


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def _triples(rng, lo, hi, n_rel, m):
    """m random triples over entities lo .. hi - 1; the last seven repeat the first seven (parallel edges)."""
    if hi <= lo or m == 0:
        return np.zeros((0, 3), np.int64)
    trip = np.stack([rng.integers(lo, hi, m), rng.integers(0, n_rel, m), rng.integers(lo, hi, m)], 1)
    return np.concatenate([trip, trip[:7]], 0)


def _subjects(rng, B, hi):
    return np.stack([np.arange(B), rng.integers(0, hi, B)], 1).astype(np.int64)


def _case(name, kind, n_ent, n_rel, B, hops, nodes0, reset="subjects", **extra):
    c = types.SimpleNamespace(name=name, kind=kind, n_ent=n_ent, n_rel=n_rel, n_rela_rows=2 * n_rel + 1, B=B, hops=hops,
                              nodes0=np.asarray(nodes0, np.int64).reshape(-1, 2), reset=reset, words=B * ((n_ent + 31) // 32),
                              bitmap_words=(B + 31) // 32, regime=None)
    for k, v in extra.items():
        setattr(c, k, v)
    return c


def regime_of(words):
    """How enqueue_expand builds a level of this many batch-major words when it is given a node buffer."""
    return "fused" if words <= SMALL_FUSED_WORDS else "split" if words <= SMALL_MAX_WORDS else "general"


def _shape_case(n_ent, B, regime, hops=3):
    """About 6 triples per entity (13 fact rows with inverses and identity), the last entity isolated where there are 31 or more,
    three hops from random subjects; with three or more queries the last one starts from the highest entity id."""
    rng = np.random.default_rng(1000 * n_ent + B)
    iso = 1 if n_ent >= 31 else 0
    nodes0 = _subjects(rng, B, n_ent - iso)
    if B >= 3:
        nodes0[-1, 1] = n_ent - 1
    return _case("e%d_b%d" % (n_ent, B), "static", n_ent, 3, B, hops, nodes0, triples=_triples(rng, 0, n_ent - iso, 3, 6 * n_ent),
                 regime=regime)


def _hub_triples(rng, n_free, hubs, n_rel):
    """Random triples over entities 0 .. n_free - 1, plus for every (hub entity, in-degree k) k - 1 triples INTO the hub from those
    entities (the identity row is its k-th in-edge; a hub is never a head, so no inverse row points at it); the last two of a hub's
    triples repeat its first two."""
    trip = [_triples(rng, 0, n_free, n_rel, 3 * n_free)]
    for hub, k in hubs:
        j = np.arange(k - 3)
        rows = np.stack([(7 * j + hub) % n_free, j % n_rel, np.full(k - 3, hub)], 1)
        trip.append(np.concatenate([rows, rows[:2]], 0))
    return np.concatenate(trip, 0)


HUB_DEGREES = (127, 128, 129, 257)


def _hub_case(name, start):
    """300 entities: 0 .. 289 random, 290 .. 293 hubs of in-degree 127 / 128 / 129 / 257 (one virtual row, exactly one, two, three),
    294 .. 299 isolated; seven random triples and two per hub are duplicated.  start: "subjects" (4 queries), "nodes" (5 queries,
    several nodes each, queries 1 and 4 none) or "empty" (no node at all)."""
    rng = np.random.default_rng(77)
    n_ent, n_free = 300, 290
    hubs = [(n_free + i, k) for i, k in enumerate(HUB_DEGREES)]
    trip = _hub_triples(rng, n_free, hubs, 4)
    if start == "subjects":
        B, nodes0 = 4, np.stack([np.arange(4), [5, 291, 299, 17]], 1)
    elif start == "nodes":
        B = 5
        per = {0: rng.choice(n_ent, 40, replace=False), 2: np.arange(n_free), 3: np.array([290, 299, 0])}
        nodes0 = np.concatenate([np.stack([np.full(len(e), b), np.sort(e)], 1) for b, e in per.items()], 0)
    else:
        B, nodes0 = 3, np.zeros((0, 2), np.int64)
    return _case(name, "static", n_ent, 4, B, 3, nodes0, reset="subjects" if start == "subjects" else "nodes", triples=trip, hubs=hubs)


def _data_rows(rng, n_ent, n_rel, m):
    """Data rows of an extrapolation graph: m random triples over all but the last entity and their inverses, shuffled; rows 20 .. 29
    repeat rows 0 .. 9 (the same (h, r, t) at several data rows)."""
    t = _triples(rng, 0, n_ent - 1, n_rel, m)[:m]
    rows = np.concatenate([t, np.stack([t[:, 2], t[:, 1] + n_rel, t[:, 0]], 1)], 0)
    rows = rows[rng.permutation(len(rows))]
    rows[20:30] = rows[0:10]
    return rows


def _quads(rows, n_ent, n_rel):
    """As the extrapolation model builds its graph: self-loops first (relation 2 n_rel, time field n_data), then the data rows, whose
    time field is their row index."""
    ent = np.arange(n_ent)
    n_data = len(rows)
    return np.concatenate([np.stack([ent, np.full(n_ent, 2 * n_rel), ent, np.full(n_ent, n_data)], 1),
                           np.column_stack([rows, np.arange(n_data)])], 0).astype(np.int64)


def _window_case(name, B, first_kind=0, n_ent=200, m=750, hops=2, seed=0):
    """Query b < 4 has window kind (first_kind + b) % 4:
        0  win_lo == win_hi (empty: only self-loops survive)
        1  [0, n_data)
        2  win_lo is the row of an out-edge of its subject (kept), win_hi = n_data
        3  win_hi is the row of an out-edge of its subject (dropped), win_lo = 0
    the others a random [lo, hi).  ``special`` lists (b, kind, row) of the kinds 2 and 3."""
    rng = np.random.default_rng(500 + 7 * B + first_kind + seed)
    n_rel = 3
    rows = _data_rows(rng, n_ent, n_rel, m)
    n_data = len(rows)
    nodes0 = _subjects(rng, B, n_ent - 1)
    lo = rng.integers(0, n_data, B)
    hi = lo + rng.integers(0, n_data - lo + 1)
    special = []
    for b in range(min(B, 4)):
        kind = (first_kind + b) % 4
        out = np.flatnonzero(rows[:, 0] == nodes0[b, 1])
        while len(out) < 3:                                        # a subject with a few out-edges
            nodes0[b, 1] = (nodes0[b, 1] + 1) % (n_ent - 1)
            out = np.flatnonzero(rows[:, 0] == nodes0[b, 1])
        if kind == 0:
            lo[b] = hi[b] = n_data // 2
        elif kind == 1:
            lo[b], hi[b] = 0, n_data
        elif kind == 2:
            lo[b], hi[b] = out[len(out) // 2], n_data
            special.append((b, 2, int(lo[b])))
        else:
            lo[b], hi[b] = 0, out[len(out) // 2]
            special.append((b, 3, int(hi[b])))
    return _case(name, "windowed", n_ent, n_rel, B, hops, nodes0, quads=_quads(rows, n_ent, n_rel), n_data=n_data, n_time=n_data + 1,
                 win_lo=lo.astype(np.int64), win_hi=hi.astype(np.int64), special=special, triples=rows[rows[:, 1] < n_rel])


def static_twin(case):
    """The static graph over a windowed case's entities (its forward data rows as triples), same queries: for the test that windows
    on a graph without row ids raise and the frontier works again afterwards."""
    return _case(case.name + "_static", "static", case.n_ent, case.n_rel, case.B, case.hops, case.nodes0, triples=case.triples)


def _bw65_windowed():
    c = _window_case("bw65_windowed", 2080, n_ent=40, m=120)
    c.regime = "split"
    return c


# (n_ent, B) -> the way the level is built when the caller hands a node buffer in
SHAPES = {(1000, 32): "fused", (1000, 33): "split", (1000, 384): "split", (1000, 385): "general", (65, 3): "fused", (97, 65): "fused",
          (1, 1): "fused", (31, 1): "fused", (32, 31): "fused", (33, 32): "fused", (64, 33): "fused"}

CASES = {
    # ---- enqueue_expand `const bool split_emit = (nodes || prev_idx) && nw > 1024;`: 1024 words, the last fused node list
    "e1000_b32": lambda: _shape_case(1000, 32, "fused"),
    # ---- the same line, 1056 words: build_level_small_kernel without a node buffer + emit_nodes_kernel
    "e1000_b33": lambda: _shape_case(1000, 33, "split"),
    # ---- enqueue_expand `if (nw <= SMALL_MAX_WORDS)`: 12288 words, the last single-workgroup level (all of its 48 KB of LDS words)
    "e1000_b384": lambda: _shape_case(1000, 384, "split"),
    # ---- the same line, 12320 words: build_level (transpose_kernel, scan, pack_kernel) + snapshot_kernel + emit_nodes_kernel
    "e1000_b385": lambda: _shape_case(1000, 385, "general"),
    # ---- build_level_small_kernel `if (2 * pair + 1 < W) words[batch * W + 2 * pair + 1] = hi;`: W = 3, the last pair has no high word
    "e65_b3": lambda: _shape_case(65, 3, "fused"),
    # ---- hop_or_kernel `while (WL < f->BW && WL < 64) WL <<= 1;`: BW = 3 -> WL = 4, one idle lane (`if (w < BW)`); W = 4
    "e97_b65": lambda: _shape_case(97, 65, "fused"),
    # ---- build_level_small_kernel `const uint32_t v = (e < n_ent) ? bitsT[...] : 0u;`: one entity, one query, 63 lanes past n_ent
    "e1_b1": lambda: _shape_case(1, 1, "fused"),
    # ---- the same line with e = 31 the only lane of the first word past n_ent; `for (int i = beg; i < end; ++i)` over nw = 1 word
    "e31_b1": lambda: _shape_case(31, 1, "fused"),
    # ---- build_level_small_kernel `if (lane < 32 && batch < B)`: B = 31, the last lane of the batch word is masked; bit 31 of W = 1
    "e32_b31": lambda: _shape_case(32, 31, "fused"),
    # ---- emit / build `make_int2(b, e0 + pos)` with e0 = 32: entity 32 is bit 0 of the second word; B = 32 fills a bitmap word
    "e33_b32": lambda: _shape_case(33, 32, "fused"),
    # ---- hop_or_kernel `atomicOr(&newT[(int64_t)t * BW + w], acc)` with BW = 2: query 32 is bit 0 of the second bitmap word
    "e64_b33": lambda: _shape_case(64, 33, "fused"),
    # ---- hop_or_kernel `for (int w0 = 0; w0 < BW; w0 += WL)`: BW = 65 > WL = 64, the loop's second pass (word 64 = queries 2048 ..)
    "bw65_static": lambda: _shape_case(40, 2080, "split", hops=2),
    # ---- hop_or_window_kernel, the same loop, and `b = w * 32 + bit` with w = 64
    "bw65_windowed": _bw65_windowed,
    # ---- hop_or_window_kernel `if (b < B && r >= win_lo[b] && r < win_hi[b]) m |= 1u << bit;`: window bounds on edge rows, an empty
    # window, B just below / at / above a multiple of 32; one query alone in each of the four kinds
    "win_b1_k0": lambda: _window_case("win_b1_k0", 1, 0),
    "win_b1_k1": lambda: _window_case("win_b1_k1", 1, 1),
    "win_b1_k2": lambda: _window_case("win_b1_k2", 1, 2),
    "win_b1_k3": lambda: _window_case("win_b1_k3", 1, 3),
    "win_b31": lambda: _window_case("win_b31", 31),
    "win_b32": lambda: _window_case("win_b32", 32),
    "win_b33": lambda: _window_case("win_b33", 33),
    "win_b65": lambda: _window_case("win_b65", 65),
    # ---- enqueue_expand `f->bm[f->level % f->n_levels]` / `bm_of(f->level - 1)`: five hops over 2 or 3 kept levels (a sparse graph:
    # the levels keep growing to the last hop)
    "ring": lambda: _shape_case_sparse("ring", 600, 5, 5),
    # ---- edge_fill_kernel `for (int j = in_ptr[t]; j < in_ptr[t + 1]; ++j)` in CSR order; hop_or_kernel's virtual rows `end = row.y +
    # row.z` at in-degree 127 / 128 / 129 / 257
    "edges_subjects": lambda: _hub_case("edges_subjects", "subjects"),
    # ---- reset_nodes_kernel + build_level on level 0 (`rg_frontier_reset_nodes`), queries without a node
    "edges_nodes": lambda: _hub_case("edges_nodes", "nodes"),
    # ---- rg_frontier_reset_nodes `if (n > 0)` and rg_frontier_edges `if (n_new == 0) return rg::zero_async(row_ptr, 4, s);`
    "edges_empty": lambda: _hub_case("edges_empty", "empty"),
}


def _shape_case_sparse(name, n_ent, B, hops):
    rng = np.random.default_rng(91)
    return _case(name, "static", n_ent, 3, B, hops, _subjects(rng, B, n_ent - 1), triples=_triples(rng, 0, n_ent - 1, 3, n_ent))


SHAPE_CASES = ["e%d_b%d" % k for k in SHAPES]
WINDOW_CASES = ["win_b1_k0", "win_b1_k1", "win_b1_k2", "win_b1_k3", "win_b31", "win_b32", "win_b33", "win_b65"]
