"""The single-source walk of rg_layer_fwd (walk 8, csrc/layer_fwd_src1.hip) called on its own, on the graph of tests/src1_ref.py: a hub
whose rows are cut and whose out-list needs several chunks, an isolated entity, a (head, tail) pair joined by three relations, and three
edges into the hub whose CSR positions lie in different segments of its row.  Random non-zero hidden[b], a_s[b], a_q.

  * agg of walk 8 equals agg of walk 1 (per-query) and walk 2 (word-parallel) at level 1 BIT FOR BIT;
  * it is within the bound of tests/test_layer_kernels_gpu.py of the fp64 edge-list reference tests/layer_ref.py;
  * the graph built on the device gives the same agg (and the same out-list) as the one built on the host;
  * walk 8 at level 2 is an error, not a launch.
Wall time on an MI355X: about 2 s."""
import numpy as np
import pytest
import torch

from tests import layer_ref as lr
from tests import src1_ref as sr

pytestmark = pytest.mark.gpu


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


@pytest.fixture(scope="module")
def graphs():
    from red_gnn_amd import engine as eng
    trip = sr.make_triples()
    host = eng.Graph(sr.N_ENT, sr.N_REL, trip)
    dev = eng.Graph.from_device(sr.N_ENT, sr.N_REL, _dev(trip, torch.int32))
    yield trip, host, dev
    host.close()
    dev.close()


def _case(trip, d, attn_dim):
    case = lr._case("src1", seed=40 + d + attn_dim, n_ent=sr.N_ENT, n_rel=sr.N_REL, B=33, hops=2, d=d, attn_dim=attn_dim, triples=trip)
    case.nodes0[:, 1] = sr.subjects()[0]
    return case


def _run(eng, case, g, X, walk):
    """agg of hop 1 with `walk` on a fresh frontier (NaN pre-fill: every row must be written); the frontier is left at level 1."""
    fr = eng.Frontier(case.n_ent, case.B, n_levels=3)
    fr.reset(_dev(case.nodes0[:, 1], torch.int32))
    n_new, n_e, n_old = fr.expand(g)
    agg = torch.full((n_new, case.ld), float("nan"), dtype=torch.float32, device="cuda")
    scratch = torch.empty(max(eng.layer_fwd_scratch_bytes(fr, g, case.ld), 256), dtype=torch.uint8, device="cuda")
    args = (X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], case.attn_dim, agg, scratch)
    eng.layer_fwd_into(fr, g, fr.level, n_new, *args, walk=walk)
    torch.cuda.synchronize()
    return agg, fr, (n_new, n_e, n_old)


def test_graph_has_the_special_entities(graphs):
    trip, host, dev = graphs
    op, ort, ip, ihr = host.export()
    assert op[sr.HUB + 1] - op[sr.HUB] > 256 and ip[sr.HUB + 1] - ip[sr.HUB] > 128
    assert op[sr.ISOLATED + 1] - op[sr.ISOLATED] == 1
    row = ort[op[sr.MULTI_HEAD]:op[sr.MULTI_HEAD + 1]]
    assert (row[:, 1] == sr.MULTI_TAIL).sum() == 3
    # the (three or more) edges 12 -> hub lie in at least two 128-entry segments of the hub's CSR-by-tail row
    hub_row = ihr[ip[sr.HUB]:ip[sr.HUB + 1]]
    at = np.flatnonzero((hub_row[:, 0] == sr.SPAN_HEAD) & (hub_row[:, 1] < sr.N_REL))
    assert len(at) >= 3 and len(set(at // 128)) >= 2


def test_out_list_order_host_and_device_build(graphs):
    """Each head's edges ordered by (tail, CSR-by-tail position): the exported arrays satisfy the property and equal the numpy build."""
    trip, host, dev = graphs
    ref_ptr, ref_rt, ref_pos, ref_ip, ref_ihr = sr.out_by_tail(trip)
    for g in (host, dev):
        op, _, ip, ihr = g.export()
        rt, pos = g.export_out_by_tail()
        sr.check_out_by_tail(op, rt, pos, ip, ihr)
        assert np.array_equal(op, ref_ptr) and np.array_equal(rt, ref_rt) and np.array_equal(pos, ref_pos)
        assert np.array_equal(ip, ref_ip) and np.array_equal(ihr, ref_ihr)


@pytest.mark.parametrize("d,attn_dim", [(64, 5), (48, 5), (64, 16), (128, 5)])
def test_walk8_bitwise_equals_walks_1_and_2_and_matches_reference(graphs, d, attn_dim):
    from red_gnn_amd import _lib, engine as eng
    trip, host, dev = graphs
    case = _case(trip, d, attn_dim)
    old, new, edges, hop = lr.hops(case)[0]
    x = lr.inputs(case, 0, hop)
    assert np.abs(x["hidden"][:, :d]).min() > 0 and np.abs(x["a_s"][:, :attn_dim]).min() > 0      # non-zero rows at level 0
    X = {k: _dev(v) for k, v in x.items() if v is not None}
    a8, fr, (n_new, n_e, n_old) = _run(eng, case, host, X, 8)
    assert (n_old, n_e, n_new) == (hop.n_old, hop.E, hop.n_new)
    assert eng.layer_fwd_walk(fr, host, 1, n_old, n_new, n_e, case.ld) == 8
    assert not torch.isnan(a8).any(), "rows never written"
    for walk in (1, 2):
        other, fr_o, _ = _run(eng, case, host, X, walk)
        assert torch.equal(a8, other), "walk 8 differs bitwise from walk %d" % walk
        fr_o.close()
    a8_dev, fr_d, _ = _run(eng, case, dev, X, 8)
    assert torch.equal(a8, a8_dev), "device-built graph"
    fr_d.close()
    # the fp64 edge-list reference, to the bound of tests/test_layer_kernels_gpu.py
    f64 = lr.forward(hop, *(x[k] for k in ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")))
    gpu = a8.cpu().numpy().astype(np.float64)
    n0 = lr.n0_of("agg", d, attn_dim)
    ratio = lr.worst_ratio(gpu, f64.agg, f64.S["agg"], f64.n["agg"], n0)
    print("src1 d=%d attn=%d (n_new %d, E %d): agg=%.3g" % (d, attn_dim, n_new, n_e, ratio))
    assert (np.abs(gpu - f64.agg) <= lr.bound(f64.S["agg"], f64.n["agg"], n0, lr.C_BOUND)).all(), ratio
    assert not a8[:, d:].any()
    # level 2: an error, not a launch (the buffer keeps its contents)
    n2, _, _ = fr.expand(host)
    canary = torch.full((n2, case.ld), 7.0, dtype=torch.float32, device="cuda")
    scratch = torch.empty(max(eng.layer_fwd_scratch_bytes(fr, host, case.ld), 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.NativeError, match="single-source walk"):
        eng.layer_fwd_into(fr, host, 2, n2, X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"],
                           case.attn_dim, canary, scratch, walk=8)
    torch.cuda.synchronize()
    assert (canary == 7.0).all()
    assert eng.layer_fwd_walk(fr, host, 2, n_new, n2, 0, case.ld) != 8
    fr.close()


def test_walk8_needs_a_frontier_started_from_subjects(graphs):
    """reset_nodes (an arbitrary node set) is not the single-source case: walk 8 is refused at level 1 too."""
    from red_gnn_amd import _lib, engine as eng
    trip, host, dev = graphs
    case = _case(trip, 64, 5)
    old, new, edges, hop = lr.hops(case)[0]
    X = {k: _dev(v) for k, v in lr.inputs(case, 0, hop).items() if v is not None}
    fr = eng.Frontier(case.n_ent, case.B, n_levels=3)
    fr.reset_nodes(_dev(case.nodes0, torch.int32))
    n_new, n_e, n_old = fr.expand(host)
    agg = torch.empty((n_new, case.ld), dtype=torch.float32, device="cuda")
    scratch = torch.empty(max(eng.layer_fwd_scratch_bytes(fr, host, case.ld), 256), dtype=torch.uint8, device="cuda")
    with pytest.raises(_lib.NativeError, match="single-source walk"):
        eng.layer_fwd_into(fr, host, 1, n_new, X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"],
                           case.attn_dim, agg, scratch, walk=8)
    fr.close()
