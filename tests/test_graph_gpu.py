"""The graph builders on the MI355X (-m gpu): every array and scalar of rg_graph_create (csrc/graph.hip), rg_graph_create_device
(csrc/graph_device.hip), rg_tgraph_create and rg_tgraph_create_excluding, copied back by Graph.export_all(), against the numpy
reference of tests/graph_ref.py over the case table defined there (each case's comment in graph_ref.CASES cites the lines it
exercises; tests/test_graph_ref.py checks the table, the reference and check_packs on the CPU).  Every comparison is an exact integer
comparison.  The packs are not compared with a rebuilt packing: graph_ref.check_packs asserts what a correct packing is.  Then the
builders' error paths, and rule_ground / rule_apply (the readers of rel_vr / rel_ht) on a device-built graph against a host-built one.
"""
import numpy as np
import pytest
import torch

from tests import graph_ref as G
from tests import rule_ground_ref as R

pytestmark = pytest.mark.gpu

# wall time of this file on an MI355X: 3.0 s (36 tests)


def _i32(x):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=torch.int32).cuda()


def _build(case, builder="host"):
    from red_gnn_amd import engine as eng
    if case.kind == "temporal":
        return eng.TemporalGraph(case.n_ent, case.n_rela_rows, case.n_time, case.quads, exclude=case.exclude)
    if builder == "host":
        return eng.Graph(case.n_ent, case.n_rel, case.triples, add_inverse=case.add_inverse)
    return eng.Graph.from_device(case.n_ent, case.n_rel, _i32(case.triples).reshape(-1, 3), add_inverse=case.add_inverse)


def _check(case, ref, graph):
    """Every array and scalar of ``graph`` equals the reference, and its packs are a correct packing; returns the export."""
    got = graph.export_all()
    assert graph.n_fact == got["n_fact"] == ref["n_fact"]
    assert G.mismatches(got, ref) == []
    if G.wants_packs(case):
        assert len(got["pack"]) > 0
        G.check_packs(ref["in_vr_rows"], ref["in_pk"], got["pack_ent"], got["pack"], got["pack_rows"])
    else:
        assert got["pack_ent"].shape == (0, 2) and got["pack"].shape == (0, 4) and got["pack_rows"].shape == (0, 2)
    return got


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("name", G.STATIC_CASES)
def test_static_graph_equals_the_reference(name, builder):
    case, ref = G.case_and_ref(name)
    graph = _build(case, builder)
    got = _check(case, ref, graph)
    if name == "packed_limit":
        # relation 4094 (the identity) is the highest: no entry reads as the padding value, so the -1 entries are the padding alone
        assert (ref["in_pk"] != 0xFFFFFFFF).all() and (ref["in_pk"] >> 20).max() == 4094 and (ref["in_pk"] & 0xFFFFF).max() == (1 << 20) - 1
        assert int((got["pack_ent"][:, 0] == -1).sum()) == len(got["pack_ent"]) - ref["n_fact"]
        assert got["in_pk"] is not None and got["out_pk"] is not None and got["out_bt_pk"] is not None
    if name == "unpacked":
        from red_gnn_amd import _lib
        assert got["in_pk"] is None and got["out_pk"] is None and got["out_bt_pk"] is None
        pk = np.empty(graph.n_fact, np.uint32)
        with pytest.raises(_lib.NativeError, match="rg_graph_export_out_by_tail: the graph's entries are not packed"):
            _lib.check(_lib.lib().rg_graph_export_out_by_tail(graph.handle, None, None, _lib.ptr(pk)))
        rt, pos = graph.export_out_by_tail()                       # ... and the unpacked out-list is still there
        assert np.array_equal(rt, ref["out_bt_rel_tail"]) and np.array_equal(pos, ref["out_bt_pos"])


@pytest.mark.parametrize("name", G.TEMPORAL_CASES)
def test_temporal_graph_equals_the_reference(name):
    from red_gnn_amd import engine as eng
    case, ref = G.case_and_ref(name)
    got = _check(case, ref, _build(case))
    assert got["out_bt_rel_tail"] is None and got["out_bt_pos"] is None and got["out_bt_pk"] is None
    if name == "t_packed_limit":
        assert got["in_pk"] is not None and (got["in_pk"] >> 20).max() == 4095 and len(got["pack"]) == 0
    if name == "t_excl_empty":                                     # an empty exclusion list: rg_tgraph_create's graph
        plain = eng.TemporalGraph(case.n_ent, case.n_rela_rows, case.n_time, case.quads).export_all()
        assert G.mismatches(plain, ref) == [] and ref["n_fact"] == len(case.quads)
    if name == "t_excl_all":                                       # no fact left: pointer arrays of zeros, every entry array empty
        assert got["n_fact"] == 0 and got["max_in_deg"] == 0 and got["max_out_deg"] == 0
        for k in ("in_ptr", "out_ptr", "rel_ptr", "time_ptr"):
            assert not got[k].any()
        for k in ("in_head_rel", "out_rel_tail", "rel_ht", "time_ht", "in_time", "out_time", "rel_tm", "time_rel", "in_pk", "out_pk"):
            assert len(got[k]) == 0
        for d in ("in", "out", "rel", "time"):
            assert not got[d + "_vr_rows"][:, 1:3].any() and len(got[d + "_vr_split"]) == 0


def test_export_all_refuses_an_unknown_name():
    from red_gnn_amd import _lib
    case, _ = G.case_and_ref("no_triples")
    graph = _build(case)
    dims = np.zeros(2, np.int64)
    with pytest.raises(_lib.NativeError, match="no array named 'in_vr'"):
        _lib.check(_lib.lib().rg_graph_export_array(graph.handle, b"in_vr", _lib.ptr(dims), None, None))


# ---- error paths ----------------------------------------------------------------------------------------------------------------------
BAD_TRIPLES = {"head": (-1, 0, 3), "rel": (3, 4, 5), "tail": (3, 0, 20)}       # n_ent = 20, n_rel = 4 with inverses: relations 0..3


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("at,what", [("first", "tail"), ("last", "rel"), ("last", "head")])
def test_a_triple_out_of_range_is_named(builder, at, what):
    from red_gnn_amd import _lib
    rng = np.random.default_rng(3)
    trip = np.stack([rng.integers(0, 20, 50), rng.integers(0, 4, 50), rng.integers(0, 20, 50)], 1)
    i = 0 if at == "first" else len(trip) - 1
    bad = trip.copy()
    bad[i] = BAD_TRIPLES[what]
    case = G._static("bad", 20, 4, bad)
    with pytest.raises(_lib.NativeError, match=r"triple %d( = \(%d,%d,%d\))? out of range" % ((i,) + BAD_TRIPLES[what])):
        _build(case, builder)
    good = G._static("good", 20, 4, trip)                          # ... and the builder still works afterwards
    _check(good, G.reference(good), _build(good, builder))


def test_an_excluded_row_out_of_range_is_refused():
    from red_gnn_amd import _lib
    from red_gnn_amd import engine as eng
    case, _ = G.case_and_ref("t_excl_dups")
    m = len(case.quads)
    for bad in (m, -1):
        with pytest.raises(_lib.NativeError, match=r"rg_tgraph_create_excluding: excluded row %d out of range \(n=%d\)" % (bad, m)):
            eng.TemporalGraph(case.n_ent, case.n_rela_rows, case.n_time, case.quads, exclude=[3, bad])


def test_a_graph_without_entities_is_refused():
    from red_gnn_amd import _lib
    from red_gnn_amd import engine as eng
    none = np.zeros((0, 3), np.int64)
    with pytest.raises(_lib.NativeError, match="rg_graph_create: n_ent=0 n_rel=3 must be positive"):
        eng.Graph(0, 3, none)
    with pytest.raises(_lib.NativeError, match="rg_graph_create_device: n_ent=0 n_rel=3 must be positive"):
        eng.Graph.from_device(0, 3, _i32(none).reshape(-1, 3))
    with pytest.raises(_lib.NativeError, match="rg_tgraph_create: n_ent=0 n_rela_rows=3 n_time=2 must be positive"):
        eng.TemporalGraph(0, 3, 2, np.zeros((0, 4), np.int64))


# ---- downstream: the kernels that read rel_vr / rel_ht, on a device-built graph ----------------------------------------------------------
def test_rule_kernels_agree_on_host_built_and_device_built_graphs():
    """rule_ground and rule_apply walk the CSR by relation through its virtual rows.  On the `lengths_inv` graph relations 5 .. 9
    (129, 255, 256, 257 and 385 facts) and their inverses 15 .. 19 are cut rows; three rules over them, the identity and relation 2
    give bitwise the same outputs on the device-built graph as on the host-built one, and the counts of the reference."""
    from red_gnn_amd import engine as eng
    case, ref = G.case_and_ref("lengths_inv")
    assert all(ref["rel_ptr"][r + 1] - ref["rel_ptr"][r] > G.VROW_MAX for r in (5, 6, 7, 8, 9, 15, 16, 17, 18, 19))
    head = np.array([5, 9, 9])
    body = np.array([[6, 18, 5], [20, 9, 20], [8, 17, 9]])
    weight = np.array([0.5, 0.25, 0.75], np.float32)
    rng = np.random.default_rng(1)
    subs, rels = rng.integers(0, case.n_ent, 70), head[rng.integers(0, 3, 70)]
    out = []
    for builder in ("host", "device"):
        graph = _build(case, builder)
        out.append((eng.rule_ground(graph, head, body), eng.rule_ground(graph, head, body, np.arange(0, case.n_ent, 3)))
                   + tuple(eng.rule_apply(graph, head, body, weight, subs, rels)))
    for a, b in zip(*out):
        assert a.dtype == b.dtype and torch.equal(a, b)
    rows = np.stack(G.static_rows(case.n_ent, case.n_rel, case.triples, True), 1)
    counts = out[1][0].cpu().numpy()
    assert np.array_equal(counts, R.counts(case.n_ent, case.n_rela_rows, rows, head, body)) and (counts > 0).all()
    fired = out[1][5].cpu().numpy()
    assert fired.any() and (fired == 0).any()
