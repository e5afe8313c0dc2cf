"""The host side of extrapolation explanation fidelity (no GPU): how RDigraph.rescore, fact_mask and data_row_mask take an extrapolation
digraph and what they refuse, with no device; fact_mask / data_row_mask on CPU tensors against tests/xrescore_ref.py; the argument
checks of T_RED_GNN.fidelity / fidelity_all, which run before anything touches a device; and the new C entry points with NULL,
negative and oversize arguments (non-zero return, rg_last_error() set, nothing enqueued)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import xrescore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REL = 6                                                  # relations 0..5 (3..5 read as inverses where a twin is asked for), identity 6

# two rows (s = 5, o = 5): 5 -r0-> 6 on days 2 and 4 at hop 1 (data rows 40, 41; row 42 is a second copy of day 2's) and back at hop 2,
# the self-loops of 5 and 6 (no data row, day = the window's first day, 0)
EDGES = [[0, 1, 5, 6, 5], [0, 1, 5, 0, 6], [0, 1, 5, 0, 6], [0, 1, 5, 0, 6], [0, 2, 5, 6, 5], [0, 2, 6, 3, 5],
         [1, 1, 5, 6, 5], [1, 1, 5, 0, 6], [1, 2, 6, 3, 5], [1, 2, 6, 4, 5]]
DAYS = [0, 2, 2, 4, 0, 2, 0, 2, 4, 2]
DATA_ROWS = [-1, 40, 42, 41, -1, 17, -1, 40, 20, 9]


def _xdigraph(B=2, n_hops=2, **kw):
    from red_gnn_amd.explain import RDigraph
    e = torch.tensor(EDGES, dtype=torch.int32).reshape(-1, 5)
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(e[:, 0].long(), minlength=B), 0)
    args = dict(edges=e, alpha=torch.full((e.shape[0],), 0.5), offsets=off, reached=torch.ones(B, dtype=torch.bool), score=torch.zeros(B),
                n_hops=n_hops, time=torch.tensor(DAYS, dtype=torch.int32), q_time=torch.tensor([5, 7], dtype=torch.int32),
                data_row=torch.tensor(DATA_ROWS, dtype=torch.int32), q_sub=torch.full((B,), 5, dtype=torch.int64),
                q_rel=torch.zeros(B, dtype=torch.int64), n_rel=N_REL)
    args.update(kw)
    return RDigraph(**args)


def _cpu_xmodel(n_layer=2, n_rel=N_REL):
    """An extrapolation.T_RED_GNN with the fields the host checks read and no device graph (its constructor builds one)."""
    from red_gnn_amd.extrapolation import T_RED_GNN
    m = T_RED_GNN.__new__(T_RED_GNN)
    torch.nn.Module.__init__(m)
    m.n_layer, m.n_rel_true, m.n_rel, m.n_ent, m.hidden_dim, m.attn_dim, m.time_granularity = n_layer, n_rel, n_rel + 1, 10, 16, 3, 24
    m.time_offset_list = np.zeros(12, np.int64)
    return m


def test_fact_mask_and_data_row_mask_against_the_reference():
    rd = _xdigraph()
    e, day, row = np.array(EDGES), np.array(DAYS), np.array(DATA_ROWS)
    T, F = True, False
    assert rd.fact_mask([(5, 0, 6, 2)]).tolist() == [F, T, T, F, F, F, F, T, F, F]                 # every copy, in every row
    assert rd.fact_mask([(5, 0, 6, 2)], inverse_offset=3).tolist() == [F, T, T, F, F, T, F, T, F, F]  # ... and the twin (6, 3, 5, 2)
    assert rd.fact_mask([(6, 3, 5, 2)]).tolist() == [F] * 5 + [T] + [F] * 4                          # the fact as given, no twin
    assert rd.fact_mask([(5, 1, 6, 2)], inverse_offset=3).tolist() == [F] * 9 + [T]                  # (6, 4, 5) is the twin of (5, 1, 6)
    assert not rd.fact_mask([(5, 0, 6, 3)], inverse_offset=3).any()                                  # another day: another fact
    assert not rd.fact_mask([(5, 6, 5, 0), (6, 6, 6, 0)], inverse_offset=3).any()                    # a self-loop is never marked
    assert not rd.fact_mask(np.zeros((0, 4), np.int64)).any()
    assert rd.fact_mask([(5, 0, 6, 2)], rows=[1]).tolist() == [F] * 7 + [T, F, F]
    m = rd.fact_mask(torch.tensor([[5, 0, 6, 40]]))                                                  # a day past every edge's
    assert m.dtype == torch.bool and m.shape == (10,) and not m.any()
    for facts, rows, off in (([(5, 0, 6, 2)], None, None), ([(5, 0, 6, 2), (5, 1, 6, 2)], [0, 1], 3), ([(6, 4, 5, 2), (5, 6, 5, 0)], [1, 1], 3),
                             ([(5, 0, 6, 2), (5, 0, 6, 4), (6, 3, 5, 4)], None, 3)):
        assert rd.fact_mask(facts, rows, off).tolist() == R.fact_mask(e, day, row, N_REL, facts, rows, off).tolist()
    assert rd.data_row_mask([40]).tolist() == [F, T, F, F, F, F, F, T, F, F]
    assert rd.data_row_mask([40, 9], rows=[1, 0]).tolist() == [F] * 7 + [T, F, F]
    assert not rd.data_row_mask(np.zeros(0, np.int64)).any() and rd.data_row_mask(torch.tensor([17, 20, 41])).sum() == 3
    for rows_, of in (([40, 42, 9], None), ([40, 9, 9], [0, 1, 0]), ([3], None)):
        assert rd.data_row_mask(rows_, of).tolist() == R.data_row_mask(e, row, rows_, of).tolist()
    # PathSet.fact_mask passes the steps' (head, rel, tail, day) through, every fact for its own row
    from red_gnn_amd.explain import PathSet
    ps = PathSet(edge=torch.tensor([[[3, 5]], [[7, 9]]]), product=torch.zeros(2, 1, dtype=torch.float64), count=torch.tensor([1, 1], dtype=torch.int32),
                 digraph=rd)
    assert ps.fact_mask(1).tolist() == [F, F, F, T, F, T, F, T, F, T]
    assert ps.fact_mask(1, inverse_offset=3).tolist() == [F, T, T, T, F, T, F, T, F, T]              # row 0 also loses the twins of (6, 3, 5, 2)


def test_masks_check_their_arguments():
    rd = _xdigraph()
    for facts, rows, off, text in (([(5, 0, 6)], None, None, r"\[F, 4\]"), ([(5.0, 0.0, 6.0, 2.0)], None, None, r"\[F, 4\]"),
                                   ([(5, 7, 6, 2)], None, None, "relation"), ([(-1, 0, 6, 2)], None, None, "negative"),
                                   ([(5, 0, 6, -2)], None, None, "negative id or day"), ([(5, 0, 6, 2)], [0, 1], None, "rows"),
                                   ([(5, 0, 6, 2)], [2], None, "rows out of range"), ([(5, 0, 6, 2)], None, 0, "inverse_offset"),
                                   ([(5, 0, 6, 2)], None, 4, "inverse_offset"), ([(5, 0, 6, 2)], None, 1.0, "inverse_offset"),
                                   ([(5, 0, 6, 2)], None, True, "inverse_offset")):
        with pytest.raises(ValueError, match=text):
            rd.fact_mask(facts, rows, off)
    for kw, missing in ((dict(q_time=None), "q_time"), (dict(q_sub=None, q_rel=None), "q_sub, q_rel"), (dict(time=None), "time"), (dict(n_rel=None), "n_rel")):
        with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.explain.*missing: " + missing):
            _xdigraph(**kw).fact_mask([(5, 0, 6, 2)])
        with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.explain.*missing: " + missing):
            _xdigraph(**kw).data_row_mask([40])
    with pytest.raises(ValueError, match="temporal.*extrapolation"):                                 # both data_row and n_time: a mix, as before
        _xdigraph(n_time=12).fact_mask([(5, 0, 6, 2)])
    for kw, text in ((dict(data_row=torch.zeros(10, dtype=torch.int64)), "data_row must be int32"), (dict(data_row=torch.zeros(9, dtype=torch.int32)), "data_row must be int32"),
                     (dict(time=torch.zeros(10, dtype=torch.int64)), "time must be int32"), (dict(q_time=torch.tensor([0, -1], dtype=torch.int32)), "negative day")):
        with pytest.raises(ValueError, match=text):
            _xdigraph(**kw).fact_mask([(5, 0, 6, 2)])
    for rows_, of, text in (([1.5], None, "data_rows must be integers"), ([[1]], None, "data_rows must be integers"), ([-1], None, "negative row"),
                            ([40], [0, 1], "rows must be integers"), ([40], [2], "rows out of range")):
        with pytest.raises(ValueError, match=text):
            rd.data_row_mask(rows_, of)
    # data_row_mask is for extrapolation digraphs only
    from tests.test_fidelity_host import EDGES as STATIC_EDGES, _digraph
    from tests.test_tfidelity_host import _tdigraph
    for other in (_digraph(STATIC_EDGES, 2), _tdigraph()):
        with pytest.raises(ValueError, match="data_row_mask: not an extrapolation r-digraph"):
            other.data_row_mask([0])


def test_rescore_dispatch_and_host_checks():
    from tests.test_fidelity_host import _cpu_model
    from tests.test_tfidelity_host import _cpu_tmodel
    model = _cpu_xmodel()
    with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.*RED_GNN_trans"):
        _xdigraph().rescore(_cpu_model())                                             # a static model
    with pytest.raises(ValueError, match=r"re-scored by the extrapolation.T_RED_GNN that explained it \(got T_RED_GNN\)"):
        _xdigraph().rescore(_cpu_tmodel())                                            # the interpolation model
    with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.*object"):
        _xdigraph().rescore(object())
    for mode in ("valid", "train", None):
        with pytest.raises(ValueError, match="extrapolation.T_RED_GNN.*mode must be 'test'"):
            _xdigraph().rescore(model, mode=mode)
    i32 = torch.int32
    for kw, text in ((dict(q_sub=None), "extrapolation.*missing: q_sub"), (dict(time=None, n_rel=None), "missing: time, n_rel"),
                     (dict(data_row=torch.zeros(10, dtype=torch.int64)), "data_row must be int32"), (dict(data_row=torch.zeros(9, dtype=i32)), "data_row must be int32"),
                     (dict(time=torch.zeros(9, dtype=i32)), "time must be int32"), (dict(q_time=torch.zeros(3, dtype=i32)), "q_time must be int32"),
                     (dict(edges=torch.tensor(EDGES)), "edges must be int32"), (dict(offsets=torch.tensor([0, 4, 9])), "offsets must start at 0"),
                     (dict(n_hops=0), "n_hops"), (dict(q_rel=torch.zeros(2, dtype=i32)), "q_rel must be int64"), (dict(n_rel=0), "n_rel")):
        with pytest.raises(ValueError, match=text):
            _xdigraph(**kw).rescore(model)
    with pytest.raises(ValueError, match="temporal.*extrapolation"):                  # data_row and n_time: a mix, today's error
        _xdigraph(n_time=12).rescore(_cpu_tmodel())
    rd = _xdigraph()
    for m, text in ((_cpu_xmodel(n_layer=3), "n_layer=3"), (_cpu_xmodel(n_rel=7), "n_rel=7")):
        with pytest.raises(ValueError, match="extrapolation.*" + text):
            rd.rescore(m)
    for keep, text in ((torch.ones(9, dtype=torch.bool), "keep must be bool or uint8 \\[10\\]"), (torch.ones(10), "keep must be bool")):
        with pytest.raises(ValueError, match=text):
            rd.rescore(model, keep=keep)
    for keep in (None, torch.ones(10, dtype=torch.bool), np.ones(10, np.uint8)):      # all in order: then the device is asked for
        with pytest.raises(ValueError, match="on one device"):
            rd.rescore(model, keep=keep)
    # an interpolation digraph handed to the extrapolation model is still the interpolation driver's to refuse
    from tests.test_tfidelity_host import _tdigraph
    with pytest.raises(ValueError, match="temporal.T_RED_GNN"):
        _tdigraph().rescore(model)


def test_fidelity_checks_its_arguments_before_anything_runs():
    from red_gnn_amd.extrapolation import T_RED_GNN, _Batch
    model = _cpu_xmodel()
    batch = _Batch(np.array([0]), np.array([0]), np.array([0]))
    good = np.array([[0, 0, 1, 24], [1, 1, 2, 48], [2, 2, 3, 72]])
    for k in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="fidelity: k"):
            model.fidelity(batch, k=k)
        with pytest.raises(ValueError, match="fidelity_all: k"):
            model.fidelity_all(good, k=k)
    for queries in (np.zeros((3, 3), np.int64), np.zeros((0, 4), np.int64), np.zeros((3, 4)), np.array([[10, 0, 0, 0]]), np.array([[0, 6, 0, 0]]),
                    np.array([[0, 0, 0, 24 * 12]])):
        with pytest.raises(ValueError, match="fidelity_all: "):
            model.fidelity_all(queries)
    for bs in (0, 1.5, True):
        with pytest.raises(ValueError, match="fidelity_all: batch_size"):
            model.fidelity_all(good, batch_size=bs)
    assert list(inspect.signature(T_RED_GNN.fidelity).parameters)[1:] == ["X", "objs", "k", "inverse_offset"]
    assert list(inspect.signature(T_RED_GNN.fidelity_all).parameters)[1:] == ["queries", "k", "batch_size", "inverse_offset"]
    from red_gnn_amd.explain import RDigraph
    assert list(inspect.signature(RDigraph.data_row_mask).parameters) == ["self", "data_rows", "rows"]


def test_header_binding_and_export():
    from red_gnn_amd import _lib, engine
    raw = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    L = _lib.lib()
    for name, n_args in (("rg_digraph_hop_ranges", 11), ("rg_digraph_hop_index_scratch_bytes", 1), ("rg_digraph_hop_index", 29)):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args == len(re.search(r"\b%s\s*\((.*?)\)" % name, text, flags=re.S).group(1).split(","))
    bits = {k: int(v) for k, v in re.findall(r"#define RG_DIGRAPH_INDEX_(\w+) (\d+)", raw)}
    assert bits == dict(ORDER=1, TWO_TAILS=2, ROW_HOP=4, ENTITY=8, RELATION=16) and sorted(b for b, _ in engine.DIGRAPH_INDEX_STATUS) == sorted(bits.values())
    assert callable(engine.digraph_hop_ranges) and callable(engine.digraph_hop_index)
    for bit, word in ((1, "ordered by"), (2, "must share their tail"), (4, "not the row of its range"), (8, "head or tail"), (16, "relation out of range")):
        assert word in str(engine.digraph_index_error(bit, "rescore", 2, 10, 3))
    assert "not the row of its range" in str(engine.digraph_index_error(1 | 2 | 4, "rescore", 2, 10, 3)) and engine.digraph_index_error(0, "x", 2, 10, 3) is None
    assert L.rg_digraph_hop_index_scratch_bytes(0) == 0 and L.rg_digraph_hop_index_scratch_bytes(-5) == 0 and L.rg_digraph_hop_index_scratch_bytes(1 << 31) == 0
    small, big = L.rg_digraph_hop_index_scratch_bytes(1), L.rg_digraph_hop_index_scratch_bytes(100000)
    assert 0 < small < big and big >= 24 * 100000 and small % 256 == 0 and big % 256 == 0


def test_argument_errors_come_before_any_launch():
    """Non-zero return and rg_last_error(); the device pointers are made-up addresses that a launch would fault on - none happens."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))

    def ranges(n_edges=9, batch=2, n_hops=2, null=(), host_null=()):
        dev = [None if i in null else fake(i) for i in range(4)]                   # 0 edges, 1 offsets, 2 hop_ptr_out, 3 hop_first_out
        ptr_h, n_h, st = np.zeros((max(batch, 1), max(n_hops, 1) + 1), np.int64), np.full(max(n_hops, 1), -7, np.int64), C.c_int32(99)
        rc = L.rg_digraph_hop_ranges(dev[0], dev[1], n_edges, batch, n_hops, dev[2], dev[3], None if 0 in host_null else _lib.ptr(ptr_h),
                                     None if 1 in host_null else _lib.ptr(n_h), None if 2 in host_null else C.byref(st), None)
        return rc, n_h, st.value

    def index(n_edges=9, batch=2, n_hops=2, hop=1, n_hop=4, n_prev=2, n_ent=10, n_rows=3, null=(), scratch=fake(30), sbytes=1 << 20, host_null=()):
        # 0 edges, 1 keep, 2 edge_time, 3 hop_ptr, 4 hop_first, 5 keys_prev, 6 at, 7 src, 8 rel, 9 time, 10 keys, 11 dst_ptr, 12 row_of, 13 prev_idx, 14 live
        dev = [None if i in null else fake(i) for i in range(15)]
        n_live, n_dst, st = C.c_int64(-7), C.c_int64(-7), C.c_int32(99)
        rc = L.rg_digraph_hop_index(dev[0], dev[1], dev[2], n_edges, batch, n_hops, hop, dev[3], dev[4], n_hop, dev[5], n_prev, n_ent, n_rows, dev[6], dev[7],
                                    dev[8], dev[9], dev[10], dev[11], dev[12], dev[13], dev[14], scratch, sbytes,
                                    None if 0 in host_null else C.byref(n_live), None if 1 in host_null else C.byref(n_dst),
                                    None if 2 in host_null else C.byref(st), None)
        return rc, n_live.value, n_dst.value, st.value

    def fails(call, text, **kw):
        assert call(**kw)[0] != 0
        assert text in L.rg_last_error().decode(), L.rg_last_error()

    fails(ranges, "n_edges=-1", n_edges=-1)
    fails(ranges, "n_edges=%d" % (1 << 31), n_edges=1 << 31)
    fails(ranges, "batch=-1", batch=-1)
    for n_hops in (0, 33, -2):
        fails(ranges, "n_hops=%d" % n_hops, n_hops=n_hops)
    for i in range(3):
        fails(ranges, "NULL argument (hop_ptr_host, hop_edges_host or status_host)", host_null=(i,))
    for i in range(4):
        fails(ranges, "NULL argument", null=(i,))
    fails(ranges, "9 edges without a row", batch=0)
    rc, n_h, st = ranges(n_edges=0, batch=0, null=range(4))                           # nothing to do is a success, whatever the pointers
    assert rc == 0 and n_h.tolist() == [0, 0] and st == 0

    fails(index, "n_edges=-1", n_edges=-1)
    fails(index, "n_edges=%d" % (1 << 31), n_edges=1 << 31)
    for hop in (0, 3, -1):
        fails(index, "hop=%d" % hop, hop=hop)
    fails(index, "n_hops=33", n_hops=33, hop=33)
    fails(index, "batch=-1", batch=-1)
    fails(index, "n_hop_edges=-1", n_hop=-1)
    fails(index, "n_hop_edges=10", n_hop=10)                                          # more than the digraph has
    fails(index, "n_prev=-1", n_prev=-1)
    fails(index, "n_prev=%d" % (1 << 31), n_prev=1 << 31)
    fails(index, "n_ent=0", n_ent=0)
    fails(index, "n_rela_rows=0", n_rows=0)
    for i in range(3):
        fails(index, "NULL argument (n_live_host, n_dst_host or status_host)", host_null=(i,))
    for i in (0, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14):
        fails(index, "NULL argument", null=(i,))
    fails(index, "edge_time and time_out go together", null=(2,))
    fails(index, "edge_time and time_out go together", null=(9,))
    fails(index, "without a row", batch=0)
    need = L.rg_digraph_hop_index_scratch_bytes(4)
    fails(index, "scratch 0 B < required %d B" % need, scratch=None, sbytes=0)
    fails(index, "scratch %d B < required %d B" % (need - 1, need), sbytes=need - 1)
    fails(index, "not 256-B aligned", scratch=C.c_void_p(0x500008))
    # nothing to do is a success, whatever the pointers: no edge in the hop, or no node one hop down
    for kw in (dict(n_hop=0), dict(n_prev=0), dict(n_hop=0, n_edges=0, batch=0)):
        assert index(null=range(15), scratch=None, sbytes=0, **kw) == (0, 0, 0, 0)
    assert index(null=(1,), n_hop=0)[0] == 0                                          # keep may be NULL
