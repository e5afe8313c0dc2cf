"""The dense frontier reference (tests/frontier_ref.py) checked on the CPU: by hand, against oracle.get_neighbors on the static cases,
against layer_ref.expand (the oracle's edges under the windows) on the temporal ones, and its case table against the conditions of
frontier.hip the GPU tests rely on (thresholds, bitmap words, virtual-row cuts, window bounds on edge rows)."""
import types

import numpy as np
import pytest

from oracle import redgnn_oracle as orc
from tests import _util as U
from tests import frontier_ref as fr
from tests import layer_ref as lr


def test_reference_on_a_graph_by_hand():
    """3 entities, 1 relation, triples (0, 0, 1), (0, 0, 1) again, (2, 0, 1).  Fact rows: 0 0->1, 1 0->1, 2 2->1, inverses 3 1->0,
    4 1->0, 5 1->2, identity 6 0->0, 7 1->1, 8 2->2.  CSR by tail: tail 0 = rows 3, 4, 6; tail 1 = rows 0, 1, 2, 7; tail 2 = rows 5, 8.
    Query 0 starts at 0, query 1 at 2 and at 1."""
    case = fr._case("hand", "static", 3, 1, 2, 1, [[0, 0], [1, 1], [1, 2]], reset="nodes", triples=[[0, 0, 1], [0, 0, 1], [2, 0, 1]])
    h, = fr.run(case)
    assert h.nodes.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [1, 2]]
    assert h.prev_idx.tolist() == [0, -1, -1, 1, 2] and h.old_new.tolist() == [0, 3, 4] and (h.n_old, h.n_new, h.E) == (3, 5, 9)
    assert h.edges.tolist() == [[0, 0, 2, 0, 0, 0],                                             # the identity row of 0
                                [0, 0, 0, 1, 0, 1], [0, 0, 0, 1, 0, 1],                         # the parallel pair, fact-row order
                                [1, 1, 1, 0, 1, 2], [1, 1, 1, 0, 1, 2],                         # their inverses
                                [1, 2, 0, 1, 2, 3], [1, 1, 2, 1, 1, 3],                         # into 1: fact row 2 before its identity row 7
                                [1, 1, 1, 2, 1, 4], [1, 2, 2, 2, 2, 4]]
    assert h.row_ptr.tolist() == [0, 1, 3, 5, 7, 9]
    assert fr.counts(case, [h]) == [(3, 0), (5, 9)]


def test_windows_by_hand():
    """2 entities, self-loops first (time field n_data = 3), then data rows 0: 0->1, 1: 0->1, 2: 1->0.  Query 0 [1, 2) keeps row 1 only;
    query 1 [0, 1) keeps row 0; query 2 [2, 2) is empty; query 3 [0, 3) starts at 1 and keeps row 2."""
    quads = [[0, 2, 0, 3], [1, 2, 1, 3], [0, 0, 1, 0], [0, 0, 1, 1], [1, 1, 0, 2]]
    case = fr._case("hand_w", "windowed", 2, 1, 4, 1, [[0, 0], [1, 0], [2, 0], [3, 1]], quads=np.array(quads), n_data=3, n_time=4,
                    win_lo=np.array([1, 0, 2, 0]), win_hi=np.array([2, 1, 2, 3]))
    h, = fr.run(case)
    assert h.nodes.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [3, 0], [3, 1]] and h.E == 7
    assert h.prev_idx.tolist() == [0, -1, 1, -1, 2, -1, 3]
    assert h.edges[:, [0, 1, 3]].tolist() == [[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1], [2, 0, 0], [3, 1, 0], [3, 1, 1]]
    free, = fr.run(case, windows=False)
    assert free.E == 3 * 3 + 2 and free.n_new == 8          # queries 0-2: loop + rows 0, 1; query 3: loop + row 2


@pytest.mark.parametrize("name", [n for n in fr.CASES if not n.startswith(("win_", "bw65_w"))])
def test_static_cases_agree_with_the_oracle(name):
    case, hops = fr.case_and_ref(name)
    og = orc.OracleGraph(orc.double_triple(case.triples, case.n_rel), case.n_ent, case.n_rel)
    nodes = case.nodes0
    for h in hops:
        t_nodes, t_edges, t_old = orc.get_neighbors(og, nodes)
        assert np.array_equal(h.nodes, t_nodes) and np.array_equal(h.old_new, t_old)
        assert (h.n_old, h.n_new, h.E) == (len(nodes), len(t_nodes), len(t_edges))
        assert np.array_equal(U.sorted_edges(h.edges), U.sorted_edges(t_edges))
        assert np.array_equal(np.diff(h.row_ptr), np.bincount(t_edges[:, 5], minlength=len(t_nodes)))
        assert np.all(np.diff(h.edges[:, 5]) >= 0)
        nodes = t_nodes


@pytest.mark.parametrize("windows", [True, False])
@pytest.mark.parametrize("name", [n for n in fr.CASES if n.startswith(("win_", "bw65_w"))])
def test_temporal_cases_agree_with_layer_ref_expand(name, windows):
    case, hops = fr.case_and_ref(name)
    if not windows:
        hops = fr.run(case, windows=False)
    og = lr.quad_graph(case.quads, case.n_ent, case.n_rela_rows)
    as_lr = types.SimpleNamespace(**dict(vars(case), kind="windowed" if windows else "temporal"))
    nodes = case.nodes0
    for h in hops:
        new, edges, erow = lr.expand(as_lr, og, nodes)
        assert np.array_equal(h.nodes, new) and h.E == len(edges) and h.n_old == len(nodes)
        assert np.array_equal(U.sorted_edges(h.edges), U.sorted_edges(edges))
        nodes = new


def test_shape_cases_land_on_the_intended_side_of_the_thresholds():
    """enqueue_expand switches at B * ceil(n_ent / 32) = 1024 (node list fused into the level build) and 12288 words (one workgroup)."""
    assert fr.regime_of(1024) == "fused" and fr.regime_of(1025) == "split" and fr.regime_of(12288) == "split" and fr.regime_of(12289) == "general"
    assert set(fr.SHAPE_CASES) <= set(fr.CASES)
    for (n_ent, B), regime in fr.SHAPES.items():
        case, _ = fr.case_and_ref("e%d_b%d" % (n_ent, B))
        assert (case.n_ent, case.B, case.hops) == (n_ent, B, 3)
        assert case.words == B * ((n_ent + 31) // 32) and fr.regime_of(case.words) == regime == case.regime, case.name
    words = {n: fr.case_and_ref(n)[0].words for n in ("e1000_b32", "e1000_b33", "e1000_b384", "e1000_b385")}
    assert words == {"e1000_b32": 1024, "e1000_b33": 1056, "e1000_b384": 12288, "e1000_b385": 12320}
    assert {r for r in fr.SHAPES.values()} == {"fused", "split", "general"}
    assert (fr.case_and_ref("e65_b3")[0].n_ent + 31) // 32 == 3                   # odd W: the last entity pair has no high word
    for name in ("bw65_static", "bw65_windowed"):                                 # more than 64 bitmap words: the word loop's second pass
        case, hops = fr.case_and_ref(name)
        assert case.bitmap_words == 65 and case.hops == 2 and fr.regime_of(case.words) == case.regime
        assert all(h.cur[2048:].sum() > 32 for h in hops)                           # ... and queries in the 65th word reach something


def test_hub_cases_sit_on_both_sides_of_the_virtual_row_cut():
    for name in ("edges_subjects", "edges_nodes", "edges_empty"):
        case, hops = fr.case_and_ref(name)
        el = fr.edge_list(case)
        indeg = np.bincount(el.tail, minlength=case.n_ent)
        assert [int(indeg[h]) for h, _ in case.hubs] == [127, 128, 129, 257] == [k for _, k in case.hubs]
        assert fr.VROW_MAX == 128 and (indeg[294:] == 1).all()                    # isolated entities: the identity row only
        trip = np.asarray(case.triples)
        assert len(np.unique(trip, axis=0)) < len(trip)                           # duplicated triples
    case, hops = fr.case_and_ref("edges_nodes")
    assert set(case.nodes0[:, 0]) == {0, 2, 3} and case.B == 5                     # queries 1 and 4 have no node
    hub_rows = np.diff(hops[0].row_ptr)[(hops[0].nodes[:, 0] == 2) & (hops[0].nodes[:, 1] >= 290) & (hops[0].nodes[:, 1] < 294)]
    assert hub_rows.tolist() == [126, 127, 128, 256]                              # every in-edge but the hub's own identity row
    case, hops = fr.case_and_ref("edges_empty")
    assert len(case.nodes0) == 0 and all(h.n_new == 0 and h.E == 0 and h.row_ptr.tolist() == [0] for h in hops)
    case, hops = fr.case_and_ref("ring")
    assert case.hops == 5 and all(a.n_new < b.n_new for a, b in zip(hops, hops[1:]))     # still growing at the fifth hop


@pytest.mark.parametrize("name", fr.WINDOW_CASES + ["bw65_windowed"])
def test_window_cases_put_their_bounds_on_edge_rows(name):
    case, hops = fr.case_and_ref(name)
    el = fr.edge_list(case)
    assert case.n_data == int((el.row < case.n_data).sum()) and (el.row[:case.n_ent] == case.n_data).all()     # self-loops first
    assert (np.sort(el.row[case.n_ent:]) == np.arange(case.n_data)).all()
    if name in fr.WINDOW_CASES:
        assert abs(case.n_ent - 200) <= 20 and abs(case.n_data - 1500) <= 100
    data = case.quads[case.n_ent:]
    assert len(np.unique(data[:, :3], axis=0)) < len(data)                          # the same (h, r, t) at several data rows
    kinds = set()
    sub = dict(case.nodes0.tolist())
    for b in range(case.B):
        lo, hi = int(case.win_lo[b]), int(case.win_hi[b])
        assert 0 <= lo <= hi <= case.n_data
        kinds.add(0 if lo == hi else 1 if (lo, hi) == (0, case.n_data) else None)
    first = hops[0]
    e1 = first.edges
    for b, kind, row in case.special:
        kinds.add(kind)
        assert data[row, 0] == sub[b] and data[row, 3] == row                       # an out-edge of the query's subject
        tail = data[row, 2]
        here = (e1[:, 0] == b) & (e1[:, 1] == sub[b]) & (e1[:, 2] == data[row, 1]) & (e1[:, 3] == tail)
        # the reference followed the row on win_lo and not the row on win_hi (counted among parallel rows of the same triple)
        same = np.flatnonzero((data[:, 0] == sub[b]) & (data[:, 1] == data[row, 1]) & (data[:, 2] == tail))
        inside = int(((same >= case.win_lo[b]) & (same < case.win_hi[b])).sum())
        assert int(here.sum()) == inside and (row in same)
        assert (case.win_lo[b] == row) if kind == 2 else (case.win_hi[b] == row)
        assert ((same == row) & (same >= case.win_lo[b]) & (same < case.win_hi[b])).any() == (kind == 2)
    want = {0, 1, 2, 3} if case.B >= 4 else {int(name[-1])}
    assert want <= kinds
    empty = [b for b in range(case.B) if case.win_lo[b] == case.win_hi[b]]
    for b in empty:                                                                 # an empty window: only the self-loops survive
        assert all((h.nodes[h.nodes[:, 0] == b][:, 1] == sub[b]).all() for h in hops)
