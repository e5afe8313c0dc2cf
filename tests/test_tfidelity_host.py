"""The host side of temporal explanation fidelity (no GPU): RDigraph.fact_mask / PathSet.fact_mask with quadruples on a hand-made temporal
digraph, the argument checks of the temporal RDigraph.rescore and T_RED_GNN.fidelity, which run before anything touches a device,
the new C symbol in the header, in _lib.SYMBOLS and in the library, and the argument errors of rg_digraph_tlayer_fwd with NULL and
made-up pointers (nothing is launched)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import trescore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REL, N_TIME, M = 6, 12, 3                              # relations 0..2, inverses 3..5, identity 6 = the model's n_rel; 12 time ids

# two rows (s = 5, o = 5): 5 -r0-> 6 at times 2 and 4 at hop 1 and back through the inverse at hop 2, the self-loops of 5 and 6 (time
# 11), and in row 1 an edge of another fact
EDGES = [[0, 1, 5, 6, 5], [0, 1, 5, 0, 6], [0, 1, 5, 0, 6], [0, 2, 5, 6, 5], [0, 2, 6, 3, 5],
         [1, 1, 5, 6, 5], [1, 1, 5, 0, 6], [1, 2, 6, 3, 5], [1, 2, 6, 4, 5]]
TIMES = [11, 2, 4, 11, 2, 11, 2, 4, 2]


def _tdigraph(B=2, n_hops=2, **kw):
    from red_gnn_amd.explain import RDigraph
    e = torch.tensor(EDGES, dtype=torch.int32).reshape(-1, 5)
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(e[:, 0].long(), minlength=B), 0)
    args = dict(edges=e, alpha=torch.full((e.shape[0],), 0.5), offsets=off, reached=torch.ones(B, dtype=torch.bool), score=torch.zeros(B),
                n_hops=n_hops, time=torch.tensor(TIMES, dtype=torch.int32), q_time=torch.tensor([2, 7], dtype=torch.int32),
                q_sub=torch.full((B,), 5, dtype=torch.int64), q_rel=torch.zeros(B, dtype=torch.int64), n_rel=N_REL, n_time=N_TIME)
    args.update(kw)
    return RDigraph(**args)


def _cpu_tmodel(n_layer=2, n_rel=N_REL, n_time=N_TIME):
    """A temporal.T_RED_GNN with the fields the host checks read and no device graph (its constructor builds one)."""
    from red_gnn_amd.temporal import T_RED_GNN
    m = T_RED_GNN.__new__(T_RED_GNN)
    torch.nn.Module.__init__(m)
    m.n_layer, m.n_rel, m.n_time, m.n_ent, m.hidden_dim, m.attn_dim, m.shared_tables = n_layer, n_rel, n_time, 10, 16, 3, False
    return m


def test_fact_mask_takes_quadruples_with_twins_on_and_off():
    rd = _tdigraph()
    e, t = np.array(EDGES), np.array(TIMES)
    assert rd.fact_mask([(5, 0, 6, 2)]).tolist() == [False, True, False, False, False, False, True, False, False]
    assert rd.fact_mask([(5, 0, 6, 2)], inverse_offset=M).tolist() == [False, True, False, False, True, False, True, False, False]
    assert rd.fact_mask([(6, 3, 5, 2)], inverse_offset=M).tolist() == [False, True, False, False, True, False, True, False, False]
    assert rd.fact_mask([(6, 3, 5, 2)]).tolist() == [False] * 4 + [True] + [False] * 4               # the quadruple as given, no twin
    assert rd.fact_mask([(5, 0, 6, 4)], inverse_offset=M).tolist() == [False, False, True] + [False] * 4 + [True, False]
    assert rd.fact_mask([(5, 1, 6, 2)], inverse_offset=M).tolist() == [False] * 8 + [True]           # (6, 4, 5) is the twin of (5, 1, 6)
    assert not rd.fact_mask([(5, 0, 6, 3)], inverse_offset=M).any()                                  # another time: another quadruple
    assert not rd.fact_mask([(5, 6, 5, 11), (6, 6, 6, 11)], inverse_offset=M).any()                  # the identity is no fact
    assert not rd.fact_mask(np.zeros((0, 4), np.int64)).any()
    assert rd.fact_mask([(5, 0, 6, 2)], rows=[1], inverse_offset=M).tolist() == [False] * 6 + [True, False, False]
    m = rd.fact_mask(torch.tensor([[5, 0, 6, 2]]))
    assert m.dtype == torch.bool and m.shape == (9,)
    for facts, rows, off in (([(5, 0, 6, 2)], None, None), ([(5, 0, 6, 2), (5, 1, 6, 2)], [0, 1], M), ([(6, 4, 5, 2), (5, 6, 5, 11)], [1, 1], M),
                             ([(5, 0, 6, 2), (5, 0, 6, 4), (6, 3, 5, 4)], None, M)):
        assert rd.fact_mask(facts, rows, off).tolist() == R.fact_mask(e, t, N_REL, facts, rows, off).tolist()


def test_fact_mask_checks_its_arguments():
    rd = _tdigraph()
    for facts, rows, off, text in (([(5, 0, 6)], None, None, r"\[F, 4\]"), ([(5.0, 0.0, 6.0, 2.0)], None, None, r"\[F, 4\]"),
                                   ([(5, 0, 6, 12)], None, None, "time id"), ([(5, 7, 6, 2)], None, None, "relation"),
                                   ([(-1, 0, 6, 2)], None, None, "negative"), ([(5, 0, 6, 2)], [0, 1], None, "rows"),
                                   ([(5, 0, 6, 2)], [2], None, "rows out of range"), ([(5, 0, 6, 2)], None, 0, "inverse_offset"),
                                   ([(5, 0, 6, 2)], None, 4, "inverse_offset"), ([(5, 0, 6, 2)], None, 1.0, "inverse_offset"),
                                   ([(5, 0, 6, 2)], None, True, "inverse_offset")):
        with pytest.raises(ValueError, match=text):
            rd.fact_mask(facts, rows, off)
    for kw, missing in ((dict(n_time=None), "n_time"), (dict(q_time=None), "q_time"), (dict(q_sub=None, q_rel=None), "q_sub, q_rel"),
                        (dict(time=None), "time")):
        with pytest.raises(ValueError, match="temporal.*missing: " + missing):
            _tdigraph(**kw).fact_mask([(5, 0, 6, 2)])
    with pytest.raises(ValueError, match="temporal.*extrapolation"):
        _tdigraph(data_row=torch.zeros(9, dtype=torch.int32)).fact_mask([(5, 0, 6, 2)])
    with pytest.raises(ValueError, match="time holds a time id"):
        _tdigraph(time=torch.full((9,), 12, dtype=torch.int32)).fact_mask([(5, 0, 6, 2)])
    # a static digraph knows its inverses
    from tests.test_fidelity_host import EDGES as STATIC_EDGES, _digraph
    with pytest.raises(ValueError, match="inverse_offset"):
        _digraph(STATIC_EDGES, 2).fact_mask([(5, 0, 6)], inverse_offset=3)
    assert _digraph(STATIC_EDGES, 2).fact_mask([(5, 0, 6)], inverse_offset=None).sum() == 4


def test_path_set_fact_mask_passes_the_quadruples_through():
    from red_gnn_amd.explain import PathSet
    rd = _tdigraph()
    # row 0: the path over the time-4 quadruple, then the self-loop path; row 1: one path, over (5, 0, 6, 2) and (6, 4, 5, 2)
    edge = torch.tensor([[[2, 4], [0, 3]], [[6, 8], [-1, -1]]])
    ps = PathSet(edge=edge, product=torch.zeros(2, 2, dtype=torch.float64), count=torch.tensor([2, 1], dtype=torch.int32), digraph=rd)
    assert ps.fact_mask(1).tolist() == [False, False, True, False, True, False, True, False, True]
    assert ps.fact_mask(2).tolist() == ps.fact_mask(1).tolist()                       # the second path of row 0 has no fact
    # with twins: row 0 also loses (5, 0, 6, 2) (the twin of its hop-2 step) but not row 1's (6, 3, 5, 4): facts count per row
    assert ps.fact_mask(1, inverse_offset=M).tolist() == [False, True, True, False, True, False, True, False, True]
    assert list(inspect.signature(PathSet.fact_mask).parameters) == ["self", "j", "inverse_offset"]
    with pytest.raises(ValueError, match="temporal.*missing: n_time"):
        PathSet(edge=edge, product=ps.product, count=ps.count, digraph=_tdigraph(n_time=None)).fact_mask(1)


def test_rescore_checks_the_temporal_digraph_on_the_host():
    from tests.test_fidelity_host import _cpu_model
    model = _cpu_tmodel()
    with pytest.raises(ValueError, match="temporal.*RED_GNN_trans"):
        _tdigraph().rescore(_cpu_model())                                             # a static model
    with pytest.raises(ValueError, match="temporal.*object"):
        _tdigraph().rescore(object())
    i32 = torch.int32
    for kw, text in ((dict(n_time=None), "temporal.*missing: n_time"), (dict(q_sub=None), "temporal.*missing: q_sub"),
                     (dict(data_row=torch.full((9,), -1, dtype=i32)), "temporal.*extrapolation"),
                     (dict(time=torch.zeros(9, dtype=torch.int64)), "time must be int32"), (dict(time=torch.zeros(8, dtype=i32)), "time must be int32"),
                     (dict(q_time=torch.zeros(3, dtype=i32)), "q_time must be int32"), (dict(time=torch.full((9,), 12, dtype=i32)), "time id"),
                     (dict(q_time=torch.tensor([0, -1], dtype=i32)), "time id"), (dict(edges=torch.tensor(EDGES)), "edges must be int32"),
                     (dict(offsets=torch.tensor([0, 4, 8])), "offsets must start at 0"), (dict(n_hops=0), "n_hops"),
                     (dict(q_rel=torch.zeros(2, dtype=i32)), "q_rel must be int64"), (dict(n_time=0), "n_time")):
        with pytest.raises(ValueError, match=text):
            _tdigraph(**kw).rescore(model)
    rd = _tdigraph()
    for m, text in ((_cpu_tmodel(n_layer=3), "n_layer=3"), (_cpu_tmodel(n_rel=7), "n_rel=7"), (_cpu_tmodel(n_time=13), "n_time=13")):
        with pytest.raises(ValueError, match="temporal.*" + text):
            rd.rescore(m)
    for mode in ("valid", "train", None):
        with pytest.raises(ValueError, match="temporal.*mode must be 'test'"):
            rd.rescore(model, mode=mode)
    for keep, text in ((torch.ones(8, dtype=torch.bool), "keep must be bool or uint8 \\[9\\]"), (torch.ones(9), "keep must be bool")):
        with pytest.raises(ValueError, match=text):
            rd.rescore(model, keep=keep)
    for keep in (None, torch.ones(9, dtype=torch.bool), np.ones(9, np.uint8)):       # all in order: then the device is asked for
        with pytest.raises(ValueError, match="on one device"):
            rd.rescore(model, keep=keep)


def test_fidelity_checks_k_before_anything_runs():
    from red_gnn_amd.temporal import T_RED_GNN
    model = _cpu_tmodel()
    batch = {"head": [0], "relation": [0], "time": [0]}
    for k in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="fidelity: k"):
            model.fidelity(batch, k=k)
        with pytest.raises(ValueError, match="fidelity_all: k"):
            model.fidelity_all(np.zeros((3, 4), np.int64), k=k)
    for quads in (np.zeros((3, 3), np.int64), np.zeros((0, 4), np.int64), np.zeros((3, 4))):
        with pytest.raises(ValueError, match="fidelity_all: quads"):
            model.fidelity_all(quads)
    with pytest.raises(ValueError, match="fidelity_all: batch_size"):
        model.fidelity_all(np.zeros((3, 4), np.int64), batch_size=0)
    assert list(inspect.signature(T_RED_GNN.fidelity).parameters)[1:] == ["batch", "objs", "k", "inverse_offset"]
    assert list(inspect.signature(T_RED_GNN.fidelity_all).parameters)[1:] == ["quads", "k", "batch_size", "inverse_offset"]


def test_header_binding_and_export():
    from red_gnn_amd import _lib, engine
    raw = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"\brg_digraph_tlayer_fwd\s*\(", text) and "rg_digraph_tlayer_fwd" in _lib.SYMBOLS
    L = _lib.lib()
    assert hasattr(L, "rg_digraph_tlayer_fwd") and len(L.rg_digraph_tlayer_fwd.argtypes) == 31 and L.rg_version() == 12
    assert len(re.search(r"\brg_digraph_tlayer_fwd\s*\((.*?)\)", text, flags=re.S).group(1).split(",")) == 31
    assert callable(engine.digraph_tlayer_fwd)


def test_argument_errors_come_before_any_launch():
    """Non-zero return and rg_last_error(); the device pointers are made-up addresses that a launch would fault on - none happens."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))
    host = lambda *v: np.array(v, np.int32)

    def call(n_dst=1, n_edges=1, ptr_h=host(0, 1), d=16, ld=16, ap=4, attn=3, n_src=4, n_rows=7, batch=2, n_time=12, n_dir=3, null=(),
             scratch=None, sbytes=0, odd=()):
        # 0 dst_ptr, 1 src_idx, 2 rel, 3 edge_time, 4 row_of_dst, 5 q_time, 6 hidden, 7 rela, 8 time_tab, 9 a_s, 10 a_r, 11 a_q, 12 w_alpha,
        # 13 b_alpha, 14 agg_out, 15 alpha_out
        dev = [None if i in null else (C.c_void_p(0x10000 * (i + 1) + 8) if i in odd else fake(i)) for i in range(16)]
        return L.rg_digraph_tlayer_fwd(n_dst, n_edges, dev[0], None if ptr_h is None else _lib.ptr(ptr_h), dev[1], dev[2], dev[3], dev[4],
                                       dev[5], n_src, n_rows, batch, n_time, n_dir, dev[6], dev[7], dev[8], d, ld, dev[9], dev[10], dev[11],
                                       ap, dev[12], dev[13], attn, dev[14], dev[15], scratch, sbytes, None)

    def fails(text, **kw):
        assert call(**kw) != 0
        assert text in L.rg_last_error().decode(), L.rg_last_error()

    for n_dir in (2, 0, 4, -1):
        fails("n_dir=%d" % n_dir, n_dir=n_dir)
    fails("n_dir=2", n_dir=2, n_dst=0, n_edges=0, ptr_h=None, null=range(16))          # ... even with nothing to do
    fails("n_time=0", n_time=0)
    fails("n_time=-3", n_time=-3)
    fails("NULL argument (edge_time, q_time or time_tab)", null=(3,))
    fails("NULL argument (edge_time, q_time or time_tab)", null=(5,))
    fails("NULL argument (edge_time, q_time or time_tab)", null=(8,))
    fails("NULL argument", ptr_h=None)
    for i in (0, 1, 2, 4, 6, 7, 9, 10, 11, 12, 13, 14):
        fails("NULL argument", null=(i,))
    fails("decreases at destination 1", n_dst=2, n_edges=2, ptr_h=host(0, 3, 2))
    fails("starts at 1", ptr_h=host(1, 1))
    fails("ends at 1, not at the number of edges 3", n_edges=3)
    for i in (6, 7, 8, 9, 10, 11, 14):                     # hidden, rela, time_tab, a_s, a_r, a_q, agg_out: float4 loads and stores
        fails("16-B aligned", odd=(i,))
    fails("16-B aligned", n_edges=300, ptr_h=host(0, 300), ld=64, d=64, scratch=C.c_void_p(0x500008), sbytes=4096)
    fails("scratch 0 B < required 1024 B", n_edges=300, ptr_h=host(0, 300), ld=64, d=64)
    for ap in (20, 24, 28):
        fails("padded attention dim %d" % ap, ap=ap, attn=17)
    fails("padded attention dim 20", ap=20, attn=17, n_edges=300, ptr_h=host(0, 300), scratch=fake(20), sbytes=1 << 20, n_dir=1)
    fails("d=16 ld=18", ld=18)
    fails("attn_dim=5 ap=4", attn=5)
    fails("edges but n_src=0", n_src=0)
    # nothing to do is a success, whatever the pointers; alpha_out may be NULL (checked with edges on the GPU)
    assert call(n_dst=0, n_edges=0, ptr_h=None, null=range(16)) == 0
    assert call(n_dst=2, n_edges=0, ptr_h=host(0, 0, 0), null=range(16), n_dir=1) == 0
