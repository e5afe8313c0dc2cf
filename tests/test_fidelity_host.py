"""The host side of explanation fidelity (no GPU): RDigraph.fact_mask / PathSet.fact_mask on hand-made digraphs, the argument checks of
RDigraph.rescore and model.fidelity, which run before anything touches a device, the new C symbols in the header, in _lib.SYMBOLS and
in the library, and the argument errors of rg_digraph_layer_fwd with NULL and made-up pointers (nothing is launched)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _util as U
from tests import rescore_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_REL = 3                                                # relations 0..2, inverses 3..5, identity 6


def _digraph(edge_list, B, n_hops=2, **kw):
    from red_gnn_amd.explain import RDigraph
    e = torch.tensor(edge_list, dtype=torch.int32).reshape(-1, 5)
    off = torch.zeros(B + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(e[:, 0].long(), minlength=B), 0)
    args = dict(edges=e, alpha=torch.full((e.shape[0],), 0.5), offsets=off, reached=torch.ones(B, dtype=torch.bool), score=torch.zeros(B),
                n_hops=n_hops, q_sub=torch.full((B,), 5, dtype=torch.int64), q_rel=torch.zeros(B, dtype=torch.int64), n_rel=N_REL)
    args.update(kw)
    return RDigraph(**args)


# two rows (s = 5, o = 5): 5 -r0-> 6 at hop 1 and back through the inverse at hop 2, the self-loops of 5 and 6, and in row 1 the fact
# 5 -r0-> 6 once more at hop 2 next to an edge of another fact
EDGES = [[0, 1, 5, 6, 5], [0, 1, 5, 0, 6], [0, 2, 5, 6, 5], [0, 2, 6, 3, 5],
         [1, 1, 5, 6, 5], [1, 1, 5, 0, 6], [1, 2, 5, 6, 5], [1, 2, 6, 3, 5], [1, 2, 6, 4, 5]]


def test_fact_mask_marks_twins_at_every_hop_and_never_a_self_loop():
    rd = _digraph(EDGES, 2)
    want = [False, True, False, True, False, True, False, True, False]
    for facts in ([(5, 0, 6)], [(6, 3, 5)], np.array([[5, 0, 6], [6, 3, 5]]), torch.tensor([[5, 0, 6]])):
        assert rd.fact_mask(facts).tolist() == want
    assert rd.fact_mask([(5, 1, 6)]).tolist() == [False] * 8 + [True]                 # (6, 4, 5) is the twin of (5, 1, 6)
    assert not rd.fact_mask([(5, 6, 5), (6, 6, 6)]).any()                             # the identity is no fact
    assert not rd.fact_mask(np.zeros((0, 3), np.int64)).any()
    assert rd.fact_mask([(5, 0, 6)], rows=[1]).tolist() == [False] * 5 + [True, False, True, False]
    assert rd.fact_mask([(5, 0, 6), (5, 1, 6)], rows=[0, 1]).tolist() == [False, True, False, True] + [False] * 4 + [True]
    m = rd.fact_mask([(5, 0, 6)])
    assert m.dtype == torch.bool and m.shape == (9,)
    for facts, rows in (([(5, 0, 6)], None), ([(5, 0, 6), (5, 1, 6)], [0, 1]), ([(6, 4, 5), (5, 6, 5)], [1, 1])):
        assert rd.fact_mask(facts, rows).tolist() == R.fact_mask(np.array(EDGES), N_REL, facts, rows).tolist()


def test_fact_mask_checks_its_arguments():
    rd = _digraph(EDGES, 2)
    for facts, rows, text in (([(5, 0)], None, "facts"), ([(5.0, 0.0, 6.0)], None, "facts"), ([(5, 7, 6)], None, "relation"),
                              ([(-1, 0, 6)], None, "negative"), ([(5, 0, 6)], [0, 1], "rows"), ([(5, 0, 6)], [2], "rows out of range")):
        with pytest.raises(ValueError, match=text):
            rd.fact_mask(facts, rows)
    with pytest.raises(ValueError, match="n_rel"):
        _digraph(EDGES, 2, n_rel=None).fact_mask([(5, 0, 6)])
    with pytest.raises(ValueError, match="temporal"):
        _digraph(EDGES, 2, time=torch.zeros(9, dtype=torch.int32)).fact_mask([(5, 0, 6)])


def test_path_set_fact_mask_takes_each_rows_best_paths():
    from red_gnn_amd.explain import PathSet
    rd = _digraph(EDGES, 2)
    # row 0: the self-loop path, then the path over the fact; row 1: one path, over the fact (6, 4, 5) = twin of (5, 1, 6)
    edge = torch.tensor([[[0, 2], [1, 3]], [[5, 8], [-1, -1]]])
    ps = PathSet(edge=edge, product=torch.zeros(2, 2, dtype=torch.float64), count=torch.tensor([2, 1], dtype=torch.int32), digraph=rd)
    assert ps.fact_mask(1).tolist() == [False] * 5 + [True, False, True, True]         # row 0's best path has no fact
    assert ps.fact_mask(2).tolist() == [False, True, False, True, False, True, False, True, True]
    for j in (0, 3, True, 1.0):
        with pytest.raises(ValueError, match="fact_mask: j"):
            ps.fact_mask(j)


def _cpu_model():
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    loader = DataLoader(ids=U.load("tiny_fwd.npz"), verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 2, 16, 3, N_REL, "relu", 0.0

    return RED_GNN_trans(P, loader)


def test_rescore_checks_the_digraph_on_the_host():
    model = _cpu_model()
    i32 = torch.int32
    for kw, text in ((dict(time=torch.zeros(9, dtype=i32)), "temporal"), (dict(q_time=torch.zeros(2, dtype=i32)), "temporal"),
                     (dict(edges=torch.tensor(EDGES)), "edges must be int32"), (dict(alpha=torch.zeros(8)), "alpha must be float32"),
                     (dict(offsets=torch.tensor([0, 4, 8])), "offsets must start at 0"), (dict(offsets=torch.tensor([0, 4, 9], dtype=i32)), "offsets must be int64"),
                     (dict(n_hops=0), "n_hops"), (dict(n_hops=3), "n_hops=3"), (dict(n_rel=None), "n_rel"), (dict(n_rel=4), "n_rel=4"),
                     (dict(q_rel=None), "q_rel"), (dict(q_sub=torch.zeros(3, dtype=torch.int64)), "q_sub")):
        with pytest.raises(ValueError, match=text):
            _digraph(EDGES, 2, **kw).rescore(model)
    rd = _digraph(EDGES, 2)
    for keep, text in ((torch.ones(8, dtype=torch.bool), "keep must be bool or uint8 \\[9\\]"), (torch.ones(9), "keep must be bool"),
                       (np.ones(9, np.int64), "keep must be bool")):
        with pytest.raises(ValueError, match=text):
            rd.rescore(model, keep=keep)
    with pytest.raises(ValueError, match="model must be"):
        rd.rescore(object())
    for keep in (None, torch.ones(9, dtype=torch.bool), np.ones(9, np.uint8)):       # all in order: then the device is asked for
        with pytest.raises(ValueError, match="on one device"):
            rd.rescore(model, keep=keep)


def test_fidelity_checks_k_before_anything_runs():
    model = _cpu_model()
    for k in (0, 9, 2.0, True):
        with pytest.raises(ValueError, match="fidelity: k"):
            model.fidelity([0], [0], k=k)
    from red_gnn_amd.models import RED_GNN_induc
    import inspect
    assert inspect.signature(RED_GNN_induc.fidelity).parameters["mode"].default == "transductive"
    assert inspect.signature(type(model).fidelity).parameters["mode"].default == "test"
    from red_gnn_amd.base_model import BaseModel
    assert list(inspect.signature(BaseModel.fidelity).parameters)[1:] == ["data", "k", "batch", "max_queries"]


def test_fidelity_methods_and_format():
    from red_gnn_amd.explain import Fidelity
    f = Fidelity(score=torch.tensor([1.0, -2.0]), without=torch.tensor([[0.25, 0.0], [-2.0, -2.0]]), only=torch.tensor([[1.0, 1.0], [0.0, 0.0]]),
                 reached_without=torch.tensor([[True, False], [True, True]]), reached_only=torch.tensor([[True, True], [False, False]]),
                 count=torch.tensor([2, 0], dtype=torch.int32), paths=None)
    assert f.necessity().tolist() == [[0.75, 1.0], [0.0, 0.0]] and f.sufficiency_gap().tolist() == [[0.0, 0.0], [-2.0, -2.0]]
    assert f.format() == ["row 0: score 1.0000 paths 2  without 0.2500 x  only 1.0000 1.0000",
                          "row 1: score -2.0000 paths 0  without -2.0000 -2.0000  only x x"]


def test_header_binding_and_export():
    from red_gnn_amd import _lib, engine
    raw = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for name in ("rg_digraph_layer_fwd", "rg_digraph_layer_fwd_scratch_bytes"):
        assert re.search(r"\b%s\s*\(" % name, text) and name in _lib.SYMBOLS
        assert hasattr(_lib.lib(), name)
    L = _lib.lib()
    assert len(L.rg_digraph_layer_fwd.argtypes) == 26 and L.rg_version() == 12
    assert int(re.search(r"#define RG_DIGRAPH_CHUNK (\d+)", raw).group(1)) == engine.DIGRAPH_CHUNK == 128
    assert os.path.exists(os.path.join(ROOT, "red-gnn_amd", "csrc", "digraph_fwd.hip")) and callable(engine.digraph_layer_fwd)
    # scratch: the chunk list (one int4 per cut destination and per chunk) and one partial row per chunk, 256-B units
    ptr = lambda *v: np.array(v, np.int32)
    sb = lambda p, ld: L.rg_digraph_layer_fwd_scratch_bytes(_lib.ptr(p), len(p) - 1, ld)
    assert sb(ptr(0, 128), 64) == 0 and sb(ptr(0, 1, 129), 64) == 0 and sb(ptr(0, 129), 64) == 256 + 2 * 256
    assert sb(ptr(0, 5, 305, 306, 1000), 20) == 256 + 256 * ((3 + 6) * 20 * 4 // 256 + 1) and sb(ptr(0, 300, 200), 64) == 0
    assert engine.digraph_chunks(ptr(0, 5, 305, 306, 1000)) == (2, 9, 694) and engine.digraph_chunks(ptr(0)) == (0, 0, 0)


def test_argument_errors_come_before_any_launch():
    """Non-zero return and rg_last_error(); the device pointers are made-up addresses that a launch would fault on - none happens."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    fake = lambda i: C.c_void_p(0x10000 * (i + 1))
    host = lambda *v: np.array(v, np.int32)

    def call(n_dst=1, n_edges=1, ptr_h=host(0, 1), d=16, ld=16, ap=4, attn=3, n_src=4, n_rows=7, batch=2, null=(), scratch=None, sbytes=0):
        dev = [None if i in null else fake(i) for i in range(13)]
        return L.rg_digraph_layer_fwd(n_dst, n_edges, dev[0], None if ptr_h is None else _lib.ptr(ptr_h), dev[1], dev[2], dev[3], n_src,
                                      n_rows, batch, dev[4], dev[5], d, ld, dev[6], dev[7], dev[8], ap, dev[9], dev[10], attn, dev[11],
                                      dev[12], scratch, sbytes, None)

    def fails(text, **kw):
        assert call(**kw) != 0
        assert text in L.rg_last_error().decode(), L.rg_last_error()

    fails("NULL argument", ptr_h=None)
    for i in range(12):                                   # every pointer but alpha_out (index 12), which may be NULL
        fails("NULL argument", null=(i,))
    fails("n_dst=-1", n_dst=-1)
    fails("n_edges=-1", n_edges=-1)
    fails("negative size", n_src=-1)
    fails("edges but n_src=0", n_src=0)
    fails("d=16 ld=18", ld=18)
    fails("d=16 ld=12", ld=12)
    fails("attn_dim=5 ap=4", attn=5)
    fails("ends at 1, not at the number of edges 3", n_edges=3)
    fails("starts at 1", ptr_h=host(1, 1))
    fails("decreases at destination 1", n_dst=2, n_edges=2, ptr_h=host(0, 3, 2))
    fails("edges without a destination", n_dst=0, n_edges=1)
    fails("scratch 0 B < required 1024 B", n_edges=300, ptr_h=host(0, 300), ld=64, d=64)
    fails("scratch 512 B < required 1024 B", n_edges=300, ptr_h=host(0, 300), ld=64, d=64, scratch=fake(20), sbytes=512)
    fails("16-B aligned", n_edges=300, ptr_h=host(0, 300), ld=64, d=64, scratch=C.c_void_p(0x500008), sbytes=4096)
    for ap in (20, 24, 28):
        fails("padded attention dim %d" % ap, ap=ap, attn=17)
    fails("padded attention dim 20", ap=20, attn=17, n_edges=300, ptr_h=host(0, 300), scratch=fake(20), sbytes=1 << 20)
    # nothing to do is a success, whatever the pointers
    assert call(n_dst=0, n_edges=0, ptr_h=None, null=range(13)) == 0
    assert call(n_dst=2, n_edges=0, ptr_h=host(0, 0, 0), null=range(13)) == 0
