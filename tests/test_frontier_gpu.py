"""The frontier (csrc/frontier.hip) called on its own - rg_frontier_reset / reset_nodes / set_window / expand / expand_async /
expand_nodes_async / nodes / level_counts / edges - against the dense set-expansion reference of tests/frontier_ref.py, over the case
table defined there (each case's comment in frontier_ref.CASES cites the line of frontier.hip it flips; tests/test_frontier_ref.py
checks the table and the reference on the CPU).  Every comparison is exact.  The node buffers the test owns hold batch * n_ent rows
pre-filled with -7: rows below the level's N must equal the reference (no -7 among them: entity ids and batch ids are >= 0, a link to
the previous level is >= -1), the rows from N on must still hold -7.
"""
import numpy as np
import pytest
import torch

from tests import frontier_ref as fref

pytestmark = pytest.mark.gpu

# wall time of this file on an MI355X: 2.7 s (77 tests)
SENTINEL = -7
FORMS = ("sync", "async", "fused")


def _i32(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).cuda()


def _graph(case):
    from red_gnn_amd import engine as eng
    if case.kind == "static":
        return eng.Graph(case.n_ent, case.n_rel, case.triples)
    return eng.TemporalGraph(case.n_ent, case.n_rela_rows, case.n_time, case.quads)


def _start(case, fr, windows=None):
    """Level 0 of the case on ``fr``; windows: set the case's row windows (default: the case is windowed)."""
    if case.kind == "windowed" if windows is None else windows:
        fr.set_window(_i32(case.win_lo), _i32(case.win_hi), case.n_data)
    if case.reset == "subjects":
        fr.reset(_i32(case.nodes0[:, 1]))
    else:
        fr.reset_nodes(_i32(case.nodes0).reshape(-1, 2))


def _buffers(case):
    cap = case.B * case.n_ent
    return (torch.full((cap, 2), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda"))


def _check_buffers(what, ref, nodes, prev):
    nodes, prev = nodes.cpu().numpy(), prev.cpu().numpy()
    n = ref.n_new
    assert np.array_equal(nodes[:n], ref.nodes), "%s: node list" % what
    assert np.array_equal(prev[:n], ref.prev_idx), "%s: links to the previous level" % what
    assert (nodes[n:] == SENTINEL).all() and (prev[n:] == SENTINEL).all(), "%s: rows past N = %d were written" % (what, n)


def _hop(what, form, fr, g, ref, n_old_known=True):
    """One hop in one of the three call forms, compared with the reference hop."""
    if form == "sync":
        n_new, n_e, n_old = fr.expand(g)
        assert (n_new, n_e) == (ref.n_new, ref.E), "%s: (N, E) = (%d, %d), reference (%d, %d)" % (what, n_new, n_e, ref.n_new, ref.E)
        assert n_old == (ref.n_old if n_old_known else -1), "%s: n_old" % what
        nodes, prev, old_new = fr.nodes(want_prev=True, want_old_new=n_old_known)
        assert np.array_equal(nodes.cpu().numpy(), ref.nodes), "%s: node list" % what
        assert np.array_equal(prev.cpu().numpy(), ref.prev_idx), "%s: links to the previous level" % what
        if n_old_known:
            assert np.array_equal(old_new.cpu().numpy(), ref.old_new), "%s: old_nodes_new_idx" % what
        return
    nodes, prev = _buffers(fr.case)
    if form == "async":
        fr.expand_async(g)
        fr.nodes_into(nodes, prev)
    else:
        fr.expand_nodes_async(g, nodes, prev)
    assert (fr.n_new, fr.n_edges) == (-1, -1)
    _check_buffers(what, ref, nodes, prev)


def _frontier(case, n_levels=2):
    from red_gnn_amd import engine as eng
    fr = eng.Frontier(case.n_ent, case.B, n_levels)
    fr.case = case
    return fr


def _walk(case, hops, fr, g, forms, what):
    """The case's hops from the level 0 ``fr`` holds, hop k in the form forms[k]; then level_counts()."""
    known = True
    for k, (ref, form) in enumerate(zip(hops, forms)):
        _hop("%s hop %d %s" % (what, k + 1, form), form, fr, g, ref, n_old_known=known)
        known = form == "sync"
    assert fr.level == len(hops)
    assert fr.level_counts() == fref.counts(case, hops), "%s: level_counts" % what


# ---- a. three call forms x three ways to build a level; b. more than 64 bitmap words per entity row -----------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", fref.SHAPE_CASES + ["bw65_static", "bw65_windowed"])
def test_call_forms_and_level_builds_give_the_reference(name, form):
    """Every hop of every form gives the reference's node list, links and (N, E) - and therefore each other's.  expand() + nodes()
    hands no node buffer to the level build; expand_async() + nodes_into() emits the list as a launch of its own; expand_nodes_async()
    fuses it into the one-workgroup level build up to 1024 words, splits it off up to 12288 and takes the general path above."""
    case, hops = fref.case_and_ref(name)
    g, fr = _graph(case), _frontier(case)
    _start(case, fr)
    _walk(case, hops, fr, g, [form] * len(hops), name)


def _captured_launches(case):
    """The number of nodes of a HIP graph that captures ONE expand_nodes_async of the case's first hop (captured, never instantiated or
    replayed: only counted).  Every fill of the library is a kernel, so the nodes are its launches."""
    import ctypes
    from red_gnn_amd import _lib
    g, fr = _graph(case), _frontier(case)
    nodes, prev = _buffers(case)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                             # warm-up on the capture conditions
        _start(case, fr)
        fr.expand_nodes_async(g, nodes, prev)
    torch.cuda.current_stream().wait_stream(side)
    _start(case, fr)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        fr.expand_nodes_async(g, nodes, prev)
    L = _lib.lib()                                                            # (dlsym through the library reaches the HIP runtime it is bound to)
    L.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    n = ctypes.c_size_t()
    assert L.hipGraphGetNodes(ctypes.c_void_p(graph.raw_cuda_graph()), None, ctypes.byref(n)) == 0
    assert L.rg_hipgraph_fill_nodes(ctypes.c_void_p(graph.raw_cuda_graph())) == 0
    _start(case, fr)                                                          # the captured hop never ran: host and device agree again
    _walk(case, fref.case_and_ref(case.name)[1], fr, g, ["fused"] * case.hops, case.name + " after the capture")
    return n.value


def test_node_list_is_fused_up_to_1024_words_and_one_workgroup_builds_up_to_12288():
    """The results of the three ways to build a level are the same (the test above), so a shifted threshold shows only in the launches:
    hop_prologue_kernel + hop_or_kernel + build_level_small_kernel = 3 up to 1024 words; + emit_nodes_kernel = 4 up to 12288 words; above
    that transpose_kernel, the scan, pack_kernel, snapshot_kernel and emit_nodes_kernel follow the two hop kernels (7 or more)."""
    n = {name: _captured_launches(fref.case_and_ref(name)[0]) for name in ("e1000_b32", "e1000_b33", "e1000_b384", "e1000_b385")}
    assert (n["e1000_b32"], n["e1000_b33"], n["e1000_b384"]) == (3, 4, 4) and n["e1000_b385"] >= 7, n


# ---- c. windows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", fref.WINDOW_CASES)
def test_windowed_hops_give_the_reference(name, form):
    """Per-query row windows with bounds ON edge rows (win_lo on a row: kept; win_hi on a row: dropped), an empty window, every row;
    E is the atomic sum hop_or_window_kernel takes."""
    case, hops = fref.case_and_ref(name)
    g, fr = _graph(case), _frontier(case)
    _start(case, fr)
    _walk(case, hops, fr, g, [form] * len(hops), name)


@pytest.mark.parametrize("name", ["win_b1_k2", "win_b33", "win_b65"])
def test_windows_can_be_taken_off_and_need_a_graph_with_row_ids(name):
    from red_gnn_amd import _lib
    case, hops = fref.case_and_ref(name)
    g, fr = _graph(case), _frontier(case)
    _start(case, fr)
    _walk(case, hops, fr, g, ["sync"] * len(hops), name)
    nodes, _, _ = fr.nodes()
    with pytest.raises(_lib.NativeError, match="windows are set"):          # the edge list of a windowed hop is not materialised
        fr.edges(g, nodes)
    # the same frontier without its windows: the unwindowed result on the same graph
    fr.set_window(None, None, 0)
    _start(case, fr, windows=False)
    free = fref.run(case, windows=False)
    assert sum(h.E for h in free) > sum(h.E for h in hops)
    _walk(case, free, fr, g, ["sync", "fused"], name + " windows off")
    # windows + a graph without row ids: an error, after which the frontier works again
    twin = fref.static_twin(case)
    gs = _graph(twin)
    _start(case, fr, windows=True)
    for expand in (lambda: fr.expand(gs), lambda: fr.expand_async(gs), lambda: fr.expand_nodes_async(gs, *_buffers(case))):
        with pytest.raises(_lib.NativeError, match="carries no data-row ids"):
            expand()
    fr.set_window(None, None, 0)
    _start(twin, fr)
    _walk(twin, fref.run(twin), fr, gs, ["async", "sync"], name + " static twin")
    e, rp = fr.edges(gs, fr.nodes(want_old_new=False)[0])                    # ... and materialises edges again
    assert e.shape[0] == int(rp[-1].item()) > 0


# ---- d. the level ring ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_levels,forms", [(2, ("sync", "async", "fused", "sync", "fused")), (3, ("async", "sync", "sync", "fused", "async")),
                                            (2, ("async",) * 5), (3, ("sync",) * 5)])
def test_level_ring_wraps_over_more_hops_than_levels(n_levels, forms):
    """Five hops over 2 or 3 kept levels (bm[level % n_levels]; the links of hop k read level k - 1 while level k overwrites the slot
    of level k - n_levels), the call forms mixed; level_counts() then lists all six levels, level 0 included."""
    case, hops = fref.case_and_ref("ring")
    g, fr = _graph(case), _frontier(case, n_levels)
    _start(case, fr)
    _walk(case, hops, fr, g, forms, "ring n_levels=%d" % n_levels)
    assert len(fr.level_counts()) == 6


# ---- e. rg_frontier_edges -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edges_subjects", "edges_nodes"])
def test_edges_in_csr_order_of_current_and_older_levels(name):
    from red_gnn_amd import _lib
    case, hops = fref.case_and_ref(name)
    g, fr = _graph(case), _frontier(case, 3)
    _start(case, fr)
    kept = {}
    for k, ref in enumerate(hops):
        _hop("%s hop %d" % (name, k + 1), "sync", fr, g, ref)
        nodes, _, _ = fr.nodes()
        edges, row_ptr = fr.edges(g, nodes)
        assert np.array_equal(edges.cpu().numpy(), ref.edges), "%s hop %d: edge rows (order included)" % (name, k + 1)
        assert np.array_equal(row_ptr.cpu().numpy(), ref.row_ptr)
        kept[k + 1] = nodes
    # level 2 is still resident with its source level 1
    edges, row_ptr = fr.edges(g, kept[2], level=2)
    assert np.array_equal(edges.cpu().numpy(), hops[1].edges) and np.array_equal(row_ptr.cpu().numpy(), hops[1].row_ptr)
    with pytest.raises(_lib.NativeError, match="not resident"):             # level 1's source, level 0, was overwritten by level 3
        fr.edges(g, kept[1], level=1)
    with pytest.raises(_lib.NativeError, match="not resident"):
        fr.edges(g, kept[3], level=4)
    with pytest.raises(_lib.NativeError, match="n_new"):                    # a node list of the wrong length
        fr.edges(g, kept[3][:-1].contiguous())
    edges, row_ptr = fr.edges(g, kept[3])                                    # still usable
    assert np.array_equal(edges.cpu().numpy(), hops[2].edges) and np.array_equal(row_ptr.cpu().numpy(), hops[2].row_ptr)
    assert fr.level_counts() == fref.counts(case, hops)


def test_an_empty_start_set_gives_empty_levels():
    """rg_frontier_reset_nodes accepts n == 0 (`nodes || n == 0`): every level is empty, counts are 0, the edge list is row_ptr = [0]."""
    case, hops = fref.case_and_ref("edges_empty")
    g, fr = _graph(case), _frontier(case, 3)
    fr.reset_nodes(torch.empty((0, 2), dtype=torch.int32, device="cuda"))
    for k, (ref, form) in enumerate(zip(hops, FORMS)):
        _hop("empty hop %d %s" % (k + 1, form), form, fr, g, ref, n_old_known=k == 0)
        if form == "sync":
            nodes, _, _ = fr.nodes()
            edges, row_ptr = fr.edges(g, nodes)
            assert edges.shape == (0, 6) and row_ptr.cpu().tolist() == [0]
    assert fr.level_counts() == [(0, 0)] * 4


# ---- f. errors leave the frontier usable ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad,msg", [([[0, 3], [5, 4]], "out of range"), ([[0, 3], [1, -1]], "out of range"), ([[0, 3], [2, 9], [0, 3]], "distinct")],
                         ids=["b_eq_B", "e_minus_1", "duplicate"])
def test_bad_start_nodes_raise_at_the_next_expand_and_the_frontier_recovers(bad, msg):
    from red_gnn_amd import _lib
    case, hops = fref.case_and_ref("ring")
    assert case.B == 5
    g, fr = _graph(case), _frontier(case)
    fr.reset_nodes(_i32(bad))
    with pytest.raises(_lib.NativeError, match=msg):
        fr.expand(g)
    _start(case, fr)
    _walk(case, hops[:2], fr, g, ["sync", "fused"], "after the error")
