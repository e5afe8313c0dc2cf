"""The host side of edge saliency (no GPU): Saliency.fact_grad / top / deletion_estimate / format on a hand-made CPU digraph, the checks
of RDigraph.saliency that run before anything touches a device, the new C symbols in the header, in _lib.SYMBOLS and in the library,
and the argument errors of rg_digraph_layer_bwd with NULL and made-up pointers (nothing is launched)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests.test_fidelity_host import EDGES, N_REL, _cpu_model, _digraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# EDGES: row 0 = loop(5) and 5 -r0-> 6 at hop 1, loop(5) and the twin 6 -r3-> 5 at hop 2; row 1 the same and 6 -r4-> 5, the twin of
# (5, 1, 6), at hop 2.  Powers of two: every sum below is exact.
GRAD = [1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, -512.0]


def _saliency(grad=GRAD, live=None):
    from red_gnn_amd.explain import Saliency
    rd = _digraph(EDGES, 2)
    live = torch.ones(9, dtype=torch.bool) if live is None else torch.tensor(live)
    return Saliency(score=torch.tensor([1.0, 2.0]), reached=torch.tensor([True, True]), live=live, alpha=torch.full((9,), 0.5),
                    edge_grad=torch.tensor(grad), digraph=rd)


def test_fact_grad_sums_both_directions_and_every_hop_and_no_self_loop():
    row, fact, grad = _saliency().fact_grad()
    assert row.tolist() == [0, 1, 1] and fact.tolist() == [[5, 0, 6], [5, 0, 6], [5, 1, 6]]
    assert grad.tolist() == [2.0 + 8.0, 32.0 + 128.0, -512.0]                        # hop 1 as (5, 0, 6), hop 2 as its twin (6, 3, 5)
    assert row.dtype == fact.dtype == torch.int64 and grad.dtype == torch.float32
    # the same grouping as fact_mask: a fact's gradient is the sum over the edges its mask marks, in its row
    s = _saliency()
    for b, f, g in zip(row.tolist(), fact.tolist(), grad.tolist()):
        assert float(s.edge_grad[s.digraph.fact_mask([f], rows=[b])].sum()) == g
    with pytest.raises(ValueError, match="inverse_offset"):
        s.fact_grad(inverse_offset=3)
    only_loops = _saliency()
    only_loops.digraph = _digraph([[0, 1, 5, 6, 5], [0, 2, 5, 6, 5]], 1)
    only_loops.edge_grad = torch.tensor([1.0, 2.0])
    assert [t.shape[0] for t in only_loops.fact_grad()] == [0, 0, 0]


def test_top_orders_by_magnitude_and_pads():
    fact, grad, count = _saliency().top(1)
    assert fact.tolist() == [[[5, 0, 6]], [[5, 1, 6]]] and grad.tolist() == [[10.0], [-512.0]] and count.tolist() == [1, 1]
    fact, grad, count = _saliency().top(3)
    assert fact.tolist() == [[[5, 0, 6], [-1, -1, -1], [-1, -1, -1]], [[5, 1, 6], [5, 0, 6], [-1, -1, -1]]]
    assert grad.tolist() == [[10.0, 0.0, 0.0], [-512.0, 160.0, 0.0]] and count.tolist() == [1, 2]
    # a tie keeps the (h, r, t) order
    tie = GRAD[:8] + [160.0]
    assert _saliency(tie).top(2)[0][1].tolist() == [[5, 0, 6], [5, 1, 6]]
    for k in (0, 1.0, True):
        with pytest.raises(ValueError, match="top: k"):
            _saliency().top(k)


def test_deletion_estimate_subtracts_the_live_masked_gradients_per_row():
    live = [True] * 7 + [False, True]                                               # edge 7 is dead: it carries no gradient to subtract
    s = _saliency(live=live)
    mask = s.digraph.fact_mask([(5, 0, 6)])
    assert s.deletion_estimate(mask).tolist() == [1.0 - (2.0 + 8.0), 2.0 - 32.0]
    assert s.deletion_estimate(mask.to(torch.uint8)).tolist() == [-9.0, -30.0] and s.deletion_estimate(mask.numpy()).tolist() == [-9.0, -30.0]
    assert s.deletion_estimate(torch.zeros(9, dtype=torch.bool)).tolist() == [1.0, 2.0]
    assert s.deletion_estimate(torch.ones(9, dtype=torch.bool)).tolist() == [1.0 - 15.0, 2.0 - (16.0 + 32.0 + 64.0 - 512.0)]
    for bad in (torch.ones(8, dtype=torch.bool), torch.ones(9), None):
        with pytest.raises(ValueError, match="deletion_estimate"):
            s.deletion_estimate(bad)


def test_format():
    s = _saliency()
    s.reached = torch.tensor([True, False])
    assert s.format() == ["row 0: score 1.0000  (5, r0, 6) +10.0000", "row 1: score x  (5, r1, 6) -512.0000  (5, r0, 6) +160.0000"]
    assert s.format(id2rel=["a", "b", "c"], k=1) == ["row 0: score 1.0000  (5, a, 6) +10.0000", "row 1: score x  (5, b, 6) -512.0000"]


def test_saliency_refuses_temporal_and_extrapolation_digraphs_and_cpu_tensors():
    model = _cpu_model()
    i32 = torch.int32
    for kw in (dict(time=torch.zeros(9, dtype=i32)), dict(time=torch.zeros(9, dtype=i32), q_time=torch.zeros(2, dtype=i32), n_time=4),
               dict(data_row=torch.zeros(9, dtype=i32), time=torch.zeros(9, dtype=i32), q_time=torch.zeros(2, dtype=i32))):
        with pytest.raises(ValueError, match="saliency: .*static and inductive models only"):
            _digraph(EDGES, 2, **kw).saliency(model)
    rd = _digraph(EDGES, 2)
    for kw, text in ((dict(n_hops=3), "saliency: .*n_hops=3"), (dict(q_rel=None), "saliency: q_rel")):
        with pytest.raises(ValueError, match=text):
            _digraph(EDGES, 2, **kw).saliency(model)
    with pytest.raises(ValueError, match="saliency: keep must be bool"):
        rd.saliency(model, keep=torch.ones(9))
    with pytest.raises(ValueError, match="saliency: model must be"):
        rd.saliency(object())
    for keep in (None, torch.ones(9, dtype=torch.bool)):                             # all in order: then the device is asked for
        with pytest.raises(ValueError, match="saliency: .*on one device"):
            rd.saliency(model, keep=keep)
    from red_gnn_amd.models import RED_GNN_induc
    assert inspect.signature(RED_GNN_induc.saliency).parameters["mode"].default == "transductive"
    assert list(inspect.signature(type(model).saliency).parameters)[1:] == ["subs", "rels", "objs", "mode"]
    assert inspect.signature(type(model).saliency).parameters["mode"].default == "test"


def test_header_binding_and_export():
    from red_gnn_amd import _lib, engine
    raw = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("rg_digraph_layer_bwd", "rg_digraph_layer_bwd_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    L = _lib.lib()
    assert len(L.rg_digraph_layer_bwd.argtypes) == 29 and len(L.rg_digraph_layer_bwd_scratch_bytes.argtypes) == 4
    assert L.rg_version() == 12
    assert os.path.exists(os.path.join(ROOT, "red-gnn_amd", "csrc", "digraph_bwd.hip")) and callable(engine.digraph_layer_bwd)
    # scratch: the chunk list (one int4 per cut source and per chunk), then one partial state row and one attention row per chunk
    ptr = lambda *v: np.array(v, np.int32)
    sb = lambda p, ld, ap: L.rg_digraph_layer_bwd_scratch_bytes(_lib.ptr(p), len(p) - 1, ld, ap)
    assert sb(ptr(0, 128), 64, 8) == 0 and sb(ptr(0, 1, 129), 64, 8) == 0 and sb(ptr(0, 300, 200), 64, 8) == 0
    assert sb(ptr(0, 129), 64, 8) == 256 + 2 * 256 + 256
    assert sb(ptr(0, 5, 305, 306, 1000), 20, 32) == 256 + 256 * ((3 + 6) * 20 * 4 // 256 + 1) + 256 * ((3 + 6) * 32 * 4 // 256 + 1)


def test_argument_errors_come_before_any_launch():
    """Non-zero return and rg_last_error(); the device pointers are made-up addresses that a launch would fault on - none happens."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))
    host = lambda *v: np.array(v, np.int32)

    def call(n_src=1, n_dst=1, n_edges=1, ptr_h=host(0, 1), d=16, ld=16, ap=4, attn=3, n_rows=7, batch=2, null=(), scratch=None, sbytes=0):
        dev = [None if i in null else fake(i) for i in range(16)]
        return L.rg_digraph_layer_bwd(n_src, n_dst, n_edges, dev[0], None if ptr_h is None else _lib.ptr(ptr_h), dev[1], dev[2], dev[3],
                                      dev[4], n_rows, batch, dev[5], dev[6], d, ld, dev[7], dev[8], dev[9], ap, dev[10], dev[11], attn,
                                      dev[12], dev[13], dev[14], dev[15], scratch, sbytes, None)

    def fails(text, **kw):
        assert call(**kw) != 0
        assert text in L.rg_last_error().decode(), L.rg_last_error()

    fails("NULL argument", ptr_h=None)
    for i in range(14):                                   # every pointer but grad_hidden and grad_a_s (14, 15), which may be NULL together
        fails("NULL argument", null=(i,))
    fails("come together", null=(14,))
    fails("come together", null=(15,))
    fails("n_src=-1", n_src=-1)
    fails("n_edges=-1", n_edges=-1)
    fails("negative size", n_rows=-1)
    fails("edges but n_dst=0", n_dst=0)
    fails("d=16 ld=18", ld=18)
    fails("d=16 ld=12", ld=12)
    fails("attn_dim=5 ap=4", attn=5)
    fails("ends at 1, not at the number of edges 3", n_edges=3)
    fails("starts at 1", ptr_h=host(1, 1))
    fails("decreases at source 1", n_src=2, n_edges=2, ptr_h=host(0, 3, 2))
    fails("edges without a source", n_src=0, n_edges=1)
    fails("scratch 0 B < required 1280 B", n_edges=300, ptr_h=host(0, 300), ld=64, d=64)
    fails("scratch 512 B < required 1280 B", n_edges=300, ptr_h=host(0, 300), ld=64, d=64, scratch=fake(20), sbytes=512)
    fails("16-B aligned", n_edges=300, ptr_h=host(0, 300), ld=64, d=64, scratch=C.c_void_p(0x500008), sbytes=4096)
    for ap in (20, 24, 28):
        fails("padded attention dim %d" % ap, ap=ap, attn=17)
    fails("padded attention dim 20", ap=20, attn=17, n_edges=300, ptr_h=host(0, 300), scratch=fake(20), sbytes=1 << 20)
    # nothing to do is a success, whatever the pointers
    assert call(n_src=0, n_edges=0, ptr_h=None, null=range(16)) == 0
    assert call(n_src=2, n_edges=0, ptr_h=host(0, 0, 0), null=range(16)) == 0
