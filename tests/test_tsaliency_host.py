"""The host side of temporal edge saliency (no GPU): Saliency.fact_grad / top / format / data_row_grad on hand-made temporal and
extrapolation digraphs with power-of-two gradients (every sum exact) against fact_mask / data_row_mask, the dispatch of
RDigraph.saliency by the model's class with what it refuses before anything touches a device, the model methods' signatures, the new
C symbol in the header, in _lib.SYMBOLS and in the library, and the argument errors of rg_digraph_tlayer_bwd with NULL and made-up
pointers (nothing is launched)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_fidelity_host import EDGES as S_EDGES, _cpu_model, _digraph
from tests.test_tfidelity_host import M, _cpu_tmodel, _tdigraph
from tests.test_xfidelity_host import DATA_ROWS, _cpu_xmodel, _xdigraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_tfidelity_host.EDGES (times TIMES): row 0 = loop(5) @11, 5 -r0-> 6 @2 and @4 at hop 1, loop(5) @11 and the twin 6 -r3-> 5 @2 at hop 2; row 1 =
# loop(5), 5 -r0-> 6 @2 at hop 1, 6 -r3-> 5 @4 and 6 -r4-> 5 @2 (the twin of (5, 1, 6, 2)) at hop 2.
T_GRAD = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, -512.0]
# test_xfidelity_host.EDGES (days DAYS, data rows DATA_ROWS): row 0 = loop, 5 -r0-> 6 on day 2 twice (rows 40, 42) and on day 4 (row 41) at hop 1, loop
# and 6 -r3-> 5 on day 2 (row 17) at hop 2; row 1 = loop, 5 -r0-> 6 day 2 (row 40), 6 -r3-> 5 day 4 (row 20), 6 -r4-> 5 day 2 (row 9).
X_GRAD = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 256.0, -1024.0]


def _sal(rd, grad):
    from red_gnn_amd.explain import Saliency
    E, B = rd.edges.shape[0], rd.offsets.numel() - 1
    return Saliency(score=torch.arange(1.0, B + 1), reached=torch.ones(B, dtype=torch.bool), live=torch.ones(E, dtype=torch.bool),
                    alpha=torch.full((E,), 0.5), edge_grad=torch.tensor(grad), digraph=rd)


def _sums_match_the_masks(s, m):
    row, fact, grad = s.fact_grad(inverse_offset=m)
    assert row.dtype == fact.dtype == torch.int64 and grad.dtype == torch.float32 and fact.shape[1] == 4
    n = 0
    for b, f, g in zip(row.tolist(), fact.tolist(), grad.tolist()):
        if m is None or f[1] < m:
            assert float(s.edge_grad[s.digraph.fact_mask([f], rows=[b], inverse_offset=m)].sum()) == g, (b, f, g)
            n += 1
    return n


def test_temporal_fact_grad_groups_like_fact_mask():
    s = _sal(_tdigraph(), T_GRAD)
    row, fact, grad = s.fact_grad()
    assert row.tolist() == [0, 0, 0, 1, 1, 1]
    assert fact.tolist() == [[5, 0, 6, 2], [5, 0, 6, 4], [6, 3, 5, 2], [5, 0, 6, 2], [6, 3, 5, 4], [6, 4, 5, 2]]      # by (row, h, r, t, time)
    assert grad.tolist() == [2.0, 4.0, 16.0, 64.0, 128.0, -512.0]                    # the identity (r = 6) is no fact
    assert _sums_match_the_masks(s, None) == 6
    row, fact, grad = s.fact_grad(inverse_offset=M)                                  # an edge with 3 <= r < 6 counts as (t, r - 3, h, time)
    assert row.tolist() == [0, 0, 1, 1, 1]
    assert fact.tolist() == [[5, 0, 6, 2], [5, 0, 6, 4], [5, 0, 6, 2], [5, 0, 6, 4], [5, 1, 6, 2]]
    assert grad.tolist() == [2.0 + 16.0, 4.0, 64.0, 128.0, -512.0]
    assert _sums_match_the_masks(s, M) == 5
    # a copy of a quadruple in its row counts once per edge, at every hop
    twice = _tdigraph()
    twice.time = torch.tensor([11, 2, 2, 11, 2, 11, 2, 4, 2], dtype=torch.int32)
    s2 = _sal(twice, T_GRAD)
    assert s2.fact_grad(inverse_offset=M)[2].tolist() == [2.0 + 4.0 + 16.0, 64.0, 128.0, -512.0] and _sums_match_the_masks(s2, M) == 4
    for bad in (0, 4, 1.0, True):
        with pytest.raises(ValueError, match="fact_grad: inverse_offset"):
            s.fact_grad(inverse_offset=bad)
    only_loops = _sal(_tdigraph(), T_GRAD)
    only_loops.digraph.edges[:, 3] = 6
    assert [t.shape for t in only_loops.fact_grad()] == [(0,), (0, 4), (0,)]
    with pytest.raises(ValueError, match="data_row_grad: not an extrapolation r-digraph"):
        s.data_row_grad()


def test_extrapolation_fact_grad_and_data_row_grad():
    s = _sal(_xdigraph(), X_GRAD)
    row, fact, grad = s.fact_grad()
    assert row.tolist() == [0, 0, 0, 1, 1, 1]
    assert fact.tolist() == [[5, 0, 6, 2], [5, 0, 6, 4], [6, 3, 5, 2], [5, 0, 6, 2], [6, 3, 5, 4], [6, 4, 5, 2]]
    assert grad.tolist() == [2.0 + 4.0, 8.0, 32.0, 128.0, 256.0, -1024.0]            # both copies of day 2's row; no self-loop
    assert _sums_match_the_masks(s, None) == 6
    row, fact, grad = s.fact_grad(inverse_offset=3)
    assert fact.tolist() == [[5, 0, 6, 2], [5, 0, 6, 4], [5, 0, 6, 2], [5, 0, 6, 4], [5, 1, 6, 2]]
    assert grad.tolist() == [2.0 + 4.0 + 32.0, 8.0, 128.0, 256.0, -1024.0] and _sums_match_the_masks(s, 3) == 5
    # an edge of a fact's relation without a data row is a self-loop: no fact
    loop = _xdigraph()
    loop.data_row = torch.tensor([-1, -1] + DATA_ROWS[2:], dtype=torch.int32)
    assert _sal(loop, X_GRAD).fact_grad()[2].tolist() == [4.0, 8.0, 32.0, 128.0, 256.0, -1024.0]
    row, data_row, grad = s.data_row_grad()
    assert row.tolist() == [0, 0, 0, 0, 1, 1, 1] and data_row.tolist() == [17, 40, 41, 42, 9, 20, 40]
    assert grad.tolist() == [32.0, 2.0, 8.0, 4.0, -1024.0, 256.0, 128.0] and row.dtype == data_row.dtype == torch.int64
    for b, r, g in zip(row.tolist(), data_row.tolist(), grad.tolist()):
        assert float(s.edge_grad[s.digraph.data_row_mask([r], rows=[b])].sum()) == g
    again = _xdigraph()
    again.data_row = torch.tensor([-1, 40, 40] + DATA_ROWS[3:], dtype=torch.int32)    # one data row behind two edges of a row
    assert _sal(again, X_GRAD).data_row_grad()[2].tolist() == [32.0, 2.0 + 4.0, 8.0, -1024.0, 256.0, 128.0]


def test_top_and_format_carry_the_time():
    s = _sal(_tdigraph(), T_GRAD)
    fact, grad, count = s.top(2)
    assert fact.shape == (2, 2, 4) and fact.tolist() == [[[6, 3, 5, 2], [5, 0, 6, 4]], [[6, 4, 5, 2], [6, 3, 5, 4]]]
    assert grad.tolist() == [[16.0, 4.0], [-512.0, 128.0]] and count.tolist() == [2, 2]
    fact, grad, count = s.top(4)
    assert fact[0, 3].tolist() == [-1, -1, -1, -1] and grad[0, 3] == 0 and count.tolist() == [3, 3]
    s.reached = torch.tensor([True, False])
    assert s.format(k=1) == ["row 0: score 1.0000  (6, r3, 5, @2) +16.0000", "row 1: score x  (6, r4, 5, @2) -512.0000"]
    assert s.format(id2rel=list("abcdefg"), k=2)[0] == "row 0: score 1.0000  (6, d, 5, @2) +16.0000  (5, a, 6, @4) +4.0000"
    x = _sal(_xdigraph(), X_GRAD)
    assert x.top(1)[0].tolist() == [[[6, 3, 5, 2]], [[6, 4, 5, 2]]] and x.format(k=1)[1] == "row 1: score 2.0000  (6, r4, 5, @2) -1024.0000"
    # a static digraph keeps its triples and its refusal
    st = _sal(_digraph(S_EDGES, 2), T_GRAD)
    assert st.top(1)[0].shape == (2, 1, 3) and st.format(k=1)[0] == "row 0: score 1.0000  (5, r0, 6) +10.0000"
    with pytest.raises(ValueError, match="inverse_offset"):
        st.fact_grad(inverse_offset=3)
    with pytest.raises(ValueError, match="data_row_grad"):
        st.data_row_grad()


def test_saliency_dispatches_on_the_models_class():
    static, tmodel, xmodel = _cpu_model(), _cpu_tmodel(), _cpu_xmodel()
    st, td, xd = _digraph(S_EDGES, 2), _tdigraph(), _xdigraph()
    # a static model keeps its path and its words
    for rd in (td, xd):
        with pytest.raises(ValueError, match="saliency: .*static and inductive models only"):
            rd.saliency(static)
    # the temporal models refuse a digraph of another family, naming it
    with pytest.raises(ValueError, match="saliency: a temporal.T_RED_GNN .*this is a static r-digraph"):
        st.saliency(tmodel)
    with pytest.raises(ValueError, match="saliency: a temporal.T_RED_GNN .*this is an extrapolation r-digraph"):
        xd.saliency(tmodel)
    with pytest.raises(ValueError, match="saliency: an extrapolation.T_RED_GNN .*this is a static r-digraph"):
        st.saliency(xmodel)
    with pytest.raises(ValueError, match="saliency: an extrapolation.T_RED_GNN .*this is a temporal interpolation r-digraph"):
        td.saliency(xmodel)
    # ... and take their own through rescore's checks, under saliency's name, up to the point where the device is asked for
    for rd, model in ((td, tmodel), (xd, xmodel)):
        with pytest.raises(ValueError, match="saliency: .*mode must be 'test'"):
            rd.saliency(model, mode="valid")
        with pytest.raises(ValueError, match="saliency: keep must be bool"):
            rd.saliency(model, keep=torch.ones(rd.edges.shape[0]))
        with pytest.raises(ValueError, match="saliency: .*on one device"):
            rd.saliency(model)
    with pytest.raises(ValueError, match="saliency: .*n_layer=3"):
        td.saliency(_cpu_tmodel(n_layer=3))
    with pytest.raises(ValueError, match="saliency: .*n_layer=3"):
        xd.saliency(_cpu_xmodel(n_layer=3))
    with pytest.raises(ValueError, match="saliency: .*missing: q_time"):
        _tdigraph(q_time=None).saliency(tmodel)
    # rescore keeps its own name
    with pytest.raises(ValueError, match="rescore: .*on one device"):
        td.rescore(tmodel)
    with pytest.raises(ValueError, match="rescore: .*on one device"):
        xd.rescore(xmodel)


def test_model_methods():
    from red_gnn_amd import explain, extrapolation, temporal
    assert list(inspect.signature(temporal.T_RED_GNN.saliency).parameters) == ["self", "batch", "objs"]
    assert list(inspect.signature(extrapolation.T_RED_GNN.saliency).parameters) == ["self", "X", "objs"]
    for cls in (temporal.T_RED_GNN, extrapolation.T_RED_GNN):
        assert inspect.signature(cls.saliency).parameters["objs"].default is None
    for f in (explain.rescore_temporal, explain.rescore_extrapolation):
        assert inspect.signature(f).parameters["tape"].default is None
        assert list(inspect.signature(f).parameters)[:4] == ["rd", "model", "keep", "mode"]
    assert "rg_digraph_tlayer_bwd" in explain.RDigraph.saliency.__doc__

    class Stub:
        def __init__(self):
            self.calls = []

        def explain(self, q, objs=None):
            self.calls.append(("explain", q, objs))
            return self

        def saliency(self, model):
            self.calls.append(("saliency", model))
            return "done"
    for cls in (temporal.T_RED_GNN, extrapolation.T_RED_GNN):                          # explain, then .saliency(model)
        stub = Stub()
        assert cls.saliency(stub, "queries", [3]) == "done" and stub.calls == [("explain", "queries", [3]), ("saliency", stub)]


def test_header_binding_and_export():
    from red_gnn_amd import _lib, engine
    raw = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\brg_digraph_tlayer_bwd\s*\(", text) and "rg_digraph_tlayer_bwd" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "rg_digraph_tlayer_bwd") and len(L.rg_digraph_tlayer_bwd.argtypes) == 34
    assert len(L.rg_digraph_layer_bwd.argtypes) == 29 and len(L.rg_digraph_layer_bwd_scratch_bytes.argtypes) == 4
    assert L.rg_version() == 12
    params = list(inspect.signature(engine.digraph_tlayer_bwd).parameters)
    assert params == ["dst_ptr", "src_idx", "rel", "row_of_dst", "hidden", "rela", "time_tab", "d", "a_s", "a_r", "a_q", "w_alpha", "b_alpha",
                      "attn_dim", "grad_agg", "edge_time", "q_time", "n_dir", "want_state"]
    assert inspect.signature(engine.digraph_tlayer_bwd).parameters["n_dir"].default == 3
    assert list(inspect.signature(engine.digraph_source_view).parameters) == ["dst_ptr", "src_idx", "n_src", "key"]
    # the scratch of the timed form is the static function's on the CSR of the directed rows
    ptr = np.array([0, 5, 305, 306, 1000, 1000, 1000], np.int32)                     # six directed rows = two sources x three
    assert L.rg_digraph_layer_bwd_scratch_bytes(_lib.ptr(ptr), 6, 20, 32) == 256 + 256 * ((3 + 6) * 20 * 4 // 256 + 1) + 256 * ((3 + 6) * 32 * 4 // 256 + 1)
    # the keyed source view on the host: a stable sort by the key
    dst_ptr = torch.tensor([0, 2, 5], dtype=torch.int32)
    src = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    key = torch.tensor([5, 1, 3, 5, 1])
    sp, sp_h, edge_of, dst_of = engine.digraph_source_view(dst_ptr, src, 6, key=key)
    assert sp.tolist() == sp_h.tolist() == [0, 0, 2, 2, 3, 3, 5] and edge_of.tolist() == [1, 4, 2, 0, 3] and dst_of.tolist() == [0, 0, 1, 1, 1]
    assert engine.digraph_source_view(dst_ptr, src, 2)[0].tolist() == [0, 2, 5]      # without a key: by source, as before
    rows = engine.digraph_directed_rows(dst_ptr, src, torch.tensor([0, 1], dtype=torch.int32), torch.tensor([3, 7, 2, 5, 9], dtype=torch.int32),
                                        torch.tensor([7, 5], dtype=torch.int32), 3)
    assert rows.tolist() == [3 * 1 + 0, 3 * 0 + 1, 3 * 1 + 0, 3 * 1 + 1, 3 * 0 + 2]
    big = engine.digraph_directed_rows(torch.tensor([0, 1], dtype=torch.int32), torch.tensor([0], dtype=torch.int32), torch.tensor([0], dtype=torch.int32),
                                       torch.tensor([2 ** 31 - 1], dtype=torch.int32), torch.tensor([-2 ** 31], dtype=torch.int32), 3)
    assert big.tolist() == [2]                                                       # a 64-bit difference
    assert engine.digraph_directed_rows(dst_ptr, src, None, None, None, 1).tolist() == src.tolist()


def test_argument_errors_come_before_any_launch():
    """Non-zero return and rg_last_error(); the device pointers are made-up addresses that a launch would fault on - none happens."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))
    host = lambda *v: np.array(v, np.int32)

    def call(n_src=1, n_dst=1, n_edges=1, ptr_h=host(0, 0, 1, 1), d=16, ld=16, ap=4, attn=3, n_rows=7, batch=2, n_time=5, n_dir=3, null=(),
             scratch=None, sbytes=0):
        dev = [None if i in null else fake(i) for i in range(19)]
        return L.rg_digraph_tlayer_bwd(n_src, n_dst, n_edges, dev[0], None if ptr_h is None else _lib.ptr(ptr_h), dev[1], dev[2], dev[3],
                                       dev[16], dev[4], dev[17], n_rows, batch, n_time, n_dir, dev[5], dev[6], dev[18], d, ld, dev[7],
                                       dev[8], dev[9], ap, dev[10], dev[11], attn, dev[12], dev[13], dev[14], dev[15], scratch, sbytes, None)

    def fails(text, **kw):
        assert call(**kw) != 0
        assert text in L.rg_last_error().decode(), L.rg_last_error()
        assert "rg_digraph_tlayer_bwd" in L.rg_last_error().decode()

    fails("NULL argument", ptr_h=None)
    for i in list(range(14)) + [16, 17, 18]:              # every pointer but grad_hidden and grad_a_s_dir (14, 15), which may be NULL together
        fails("NULL argument", null=(i,))
    fails("come together", null=(14,))
    fails("come together", null=(15,))
    assert call(null=(14, 15), n_edges=0, ptr_h=host(0, 0, 0, 0)) == 0
    fails("n_dir=2", n_dir=2)
    fails("n_dir=0", n_dir=0)
    fails("n_time=0", n_time=0)
    fails("n_time=-3", n_time=-3)
    fails("n_time=1073741824", n_time=1 << 30)            # three tables of 2^30 rows
    fails("three rows each overflow int32", n_src=1 << 30, ptr_h=host(0, 1))
    fails("three rows each overflow int32", n_rows=1 << 30)
    fails("n_src=-1", n_src=-1)
    fails("n_edges=-1", n_edges=-1)
    fails("negative size", n_rows=-1)
    fails("edges but n_dst=0", n_dst=0)
    fails("d=16 ld=18", ld=18)
    fails("d=16 ld=12", ld=12)
    fails("attn_dim=5 ap=4", attn=5)
    # the CSR has n_dir * n_src + 1 entries
    fails("ends at 1, not at the number of edges 3", n_edges=3)
    fails("ends at 0, not at the number of edges 1", ptr_h=host(0, 0, 0, 0))
    fails("starts at 1", ptr_h=host(1, 1, 1, 1))
    fails("decreases at source 1", n_edges=2, ptr_h=host(0, 3, 2, 2))
    fails("decreases at source 4", n_src=2, n_edges=2, ptr_h=host(0, 0, 1, 2, 3, 2, 2))
    fails("edges without a source", n_src=0, n_edges=1)
    fails("scratch 0 B < required 1280 B", n_edges=300, ptr_h=host(0, 0, 300, 300), ld=64, d=64)
    fails("scratch 512 B < required 1280 B", n_edges=300, ptr_h=host(0, 300), n_dir=1, ld=64, d=64, scratch=fake(20), sbytes=512)
    fails("16-B aligned", n_edges=300, ptr_h=host(0, 300, 300, 300), ld=64, d=64, scratch=C.c_void_p(0x500008), sbytes=4096)
    for ap in (20, 24, 28):
        fails("padded attention dim %d" % ap, ap=ap, attn=17)
    fails("padded attention dim 20", ap=20, attn=17, n_edges=300, ptr_h=host(0, 300, 300, 300), scratch=fake(20), sbytes=1 << 20)
    # nothing to do is a success, whatever the pointers
    assert call(n_src=0, n_edges=0, ptr_h=None, null=range(19)) == 0
    assert call(n_src=2, n_edges=0, ptr_h=host(0, 0, 0, 0, 0, 0, 0), null=range(19)) == 0
    assert call(n_src=2, n_edges=0, n_dir=1, ptr_h=host(0, 0, 0), null=range(19)) == 0
