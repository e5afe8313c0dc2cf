"""rg_digraph_tlayer_bwd called on its own (-m gpu): the adjoint of one timed edge-list hop, in both forms (n_dir = 3 and n_dir = 1), with
respect to the gates, the directed source states and the attention rows per directed source, against the fp64 per-edge reference of
tests/digraph_tbwd_ref.py under tests/layer_ref.py's error model unchanged:

    |out - ref64| <= C_BOUND * (n + n0) * u * S + 1e-30            (layer_ref's docstring defines S, n, n0; C_BOUND = 1.6; grad_gate's S, n
                                                                    and n0: digraph_tbwd_ref's docstring)

The edge lists are the CPU oracle's temporal and windowed hops (layer_ref) in destination order, plus hand-built lists: hub rows, times
outside the table, one edge.  Every element of every output is checked, pad columns included; the outputs are pre-filled with NaN
(every row must be written), two runs are bit-equal, and grad_gate keeps its bits without the state outputs.
The kernel's worst ratios over these cases, as measured on an MI355X: 0.07 for grad_gate, 0.17 for grad_hidden, 0.022 for grad_a_s_dir
(information only, the assertions use C_BOUND).  Wall time of this file there: 3.7 s (26 tests).
"""
import numpy as np
import pytest
import torch

from tests import digraph_tbwd_ref as T
from tests import layer_ref as lr

pytestmark = pytest.mark.gpu


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _inputs(c, k, hop):
    x = T.inputs(c, k, hop)
    return x, {kk: _dev(v) for kk, v in x.items() if v is not None}


def _call(c, hop, A, X, ap=None, attn=None, want_state=True, V=None):
    """The raw entry point on numpy index arrays ``A`` (the forward's, with edge_time) and the directed view of ``hop``, and device
    inputs ``X``: (grad_gate, grad_hidden, grad_a_s_dir) pre-filled with NaN (the last two None without ``want_state``)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    V = T.directed_view(hop) if V is None else V
    n_dir, n_src, n_dst, E = hop.n_dir, hop.n_old, len(A["dst_ptr"]) - 1, len(A["src_idx"])
    n_rows = n_dir * n_src
    ap = c.ap if ap is None else ap
    I = {k: _dev(v, torch.int32) for k, v in {**A, **V, "q_time": c.q_time}.items()}
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    gate, gh, gas = nan(E), nan(n_rows, c.ld) if want_state else None, nan(n_rows, ap) if want_state else None
    nb = L.rg_digraph_layer_bwd_scratch_bytes(p(V["src_ptr"]), n_rows, c.ld, ap) if n_rows else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    assert X["hidden"].shape[0] == n_rows and X["rela"].shape[0] == n_dir * c.n_rela_rows and X["time_tab"].shape[0] == n_dir * c.n_tab_rows
    _lib.check(L.rg_digraph_tlayer_bwd(n_src, n_dst, E, p(I["src_ptr"]), p(V["src_ptr"]), p(I["edge_of"]), p(I["dst_of_edge"]), p(I["rel"]),
                                       p(I["edge_time"]), p(I["row_of_dst"]), p(I["q_time"]), c.n_rela_rows, X["a_q"].shape[0],
                                       c.n_tab_rows, n_dir, p(X["hidden"]), p(X["rela"]), p(X["time_tab"]), c.d, c.ld, p(X["a_s"]),
                                       p(X["a_r"]), p(X["a_q"]), ap, p(X["w_alpha"]), p(X["b_alpha"]), c.attn_dim if attn is None else attn,
                                       p(X["grad_agg"]), p(gate), p(gh), p(gas), p(scratch), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return gate, gh, gas


def _check(tag, c, got, f64):
    for name, t in zip(T.OUTPUTS, got):
        g = t.cpu().numpy().astype(np.float64)
        assert not np.isnan(g).any(), "%s: %d elements of %s were never written" % (tag, int(np.isnan(g).sum()), name)
        ref, n0 = getattr(f64, name), T.n0_of(name, c.d, c.attn_dim)
        ok = np.abs(g - ref) <= lr.bound(f64.S[name], f64.n[name], n0, lr.C_BOUND)
        ratio = lr.worst_ratio(g, ref, f64.S[name], f64.n[name], n0)
        print("%s %s: worst ratio %.3g (allowed %.3g)" % (tag, name, ratio, lr.C_BOUND))
        assert ok.all(), "%s %s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g)" % (tag, name, int((~ok).sum()), ok.size,
                                                                                                       ratio, lr.C_BOUND)
    assert not got[2][:, c.attn_dim:].any(), tag + ": pad columns of grad_a_s_dir"


def _run_hop(tag, c, k, hop, A):
    """One hop: the kernel against the reference, two runs bit for bit, and the gate gradients alone (NULL state outputs)."""
    x, X = _inputs(c, k, hop)
    got = _call(c, hop, A, X)
    _check(tag, c, got, T.backward(hop, *T.tables(x)))
    again = _call(c, hop, A, X)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), tag + ": two runs differ"
    gate, none_h, none_as = _call(c, hop, A, X, want_state=False)
    assert none_h is None and none_as is None and torch.equal(gate, got[0]), tag + ": grad_gate without the state outputs"
    if c.d < c.ld:                  # layer_ref's grad_agg fills its pad columns; with them zero, those of grad_hidden are zero
        G = X["grad_agg"].clone()
        G[:, c.d:] = 0
        padded = _call(c, hop, A, dict(X, grad_agg=G))
        assert not padded[1][:, c.d:].any() and torch.equal(padded[1][:, :c.d], got[1][:, :c.d]), tag + ": pad columns of grad_hidden"
    empty = torch.as_tensor(np.diff(T.directed_view(hop)["src_ptr"]) == 0).cuda()
    assert not got[1][empty].any() and not got[2][empty].any(), tag + ": a directed row without edges is not zero"
    return X, got


def _run_case(c):
    for k, hop, A in T.case_hops(c):
        _run_hop("%s hop %d" % (c.name, k + 1), c, k, hop, A)


@pytest.mark.parametrize("n_dir", T.N_DIRS)
@pytest.mark.parametrize("d,ld", T.ROW_WIDTHS)
def test_row_widths(d, ld, n_dir):
    _run_case(T.row_width_case(n_dir, d, ld))


@pytest.mark.parametrize("n_dir", T.N_DIRS)
@pytest.mark.parametrize("attn,ap", T.ATTENTION_WIDTHS)
def test_attention_widths(attn, ap, n_dir):
    _run_case(T.attention_case(n_dir, attn, ap))


@pytest.mark.parametrize("n_dir", T.N_DIRS)
def test_hub_rows_next_to_many_one_edge_rows(n_dir):
    """Directed rows of 0, 1, 127, 128, 129, 256, 257 and 3000 edges (3000: 24 chunks; 128: the longest that is not cut) among a
    thousand one-edge rows; n_dir = 3: sources 0 and 2 have edges in exactly two of three directions, and their empty directed row is
    written as zeros.  A row's outputs and its edges' gate gradients do not depend on what else the call carries: the hubs alone,
    and every third row, give bit for bit those of the full call."""
    from red_gnn_amd import engine
    c, hop, A = T.hub_hop(n_dir)
    X, (gate, gh, gas) = _run_hop(c.name, c, 0, hop, A)
    V = T.directed_view(hop)
    deg = np.diff(V["src_ptr"].astype(np.int64))
    assert engine.digraph_chunks(V["src_ptr"]) == (4, 2 + 2 + 3 + 24, 3000) and (deg == 1).sum() >= 1000 and (deg == engine.DIGRAPH_CHUNK).any()
    for u in (0, 8):                                                                  # the rows without edges, next to rows with some
        assert deg[u] == 0 and not gh[u].any() and not gas[u].any()
    assert gh[1].any() and gh[7].any()
    for pick in (np.nonzero(deg > engine.DIGRAPH_CHUNK)[0], np.arange(0, len(deg), 3), np.array([int(deg.argmax())])):
        A2, at = T.take_rows(A, hop, pick)
        hop2 = T.timed_hop(A2, c.q_time, n_dir, hop.n_old, c.n_rela_rows, c.n_tab_rows)
        g2, h2, as2 = _call(c, hop2, A2, X)
        rows = torch.as_tensor(pick).cuda()
        assert torch.equal(g2, gate[torch.as_tensor(at).cuda()]) and torch.equal(h2[rows], gh[rows]) and torch.equal(as2[rows], gas[rows]), \
            "a directed row's gradients depend on the rest of the call"
        other = torch.ones(len(deg), dtype=torch.bool, device="cuda")
        other[rows] = False
        assert not h2[other].any() and not as2[other].any()


@pytest.mark.parametrize("n_dir", T.N_DIRS)
def test_times_outside_the_table_are_clamped(n_dir):
    """n_dir = 3: |dt| >= n_time on both sides; n_dir = 1: a negative lag and one past the table.  The reference clamps as the header
    says the kernel does; the moved edges carry a gradient."""
    c, k, hop, A, at = T.clamped_hop(n_dir)
    _, got = _run_hop(c.name, c, k, hop, A)
    assert bool((got[0][torch.as_tensor(at).cuda()] != 0).all())


@pytest.mark.parametrize("n_dir", T.N_DIRS)
def test_one_source_with_one_edge(n_dir):
    c, hop, A = T.one_edge_hop(n_dir)
    x, X = _inputs(c, 0, hop)
    got = _call(c, hop, A, X)
    _check("one edge", c, got, T.backward(hop, *T.tables(x)))
    u = int(hop.hrow[0])
    rest = np.arange(n_dir * hop.n_old) != u
    assert got[0].shape == (1,) and float(got[0][0]) != 0.0 and got[1][u].any() and not got[1][torch.as_tensor(rest).cuda()].any()


def _engine_args(c, A, X):
    I = {kk: _dev(v, torch.int32) for kk, v in {**A, "q_time": c.q_time}.items()}
    tabs = (X["hidden"], X["rela"], X["time_tab"], c.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], c.attn_dim, X["grad_agg"])
    return I, tabs


@pytest.mark.parametrize("n_dir", T.N_DIRS)
def test_engine_wrapper_checks_and_matches(n_dir):
    """engine.digraph_tlayer_bwd builds the directed view itself: the raw call's bits (the attention rows added per source in the
    order past, now, future), None state outputs on request, E == 0, and ValueError for indices outside their tables and shapes
    that do not fit."""
    from red_gnn_amd import engine
    c = T.case("wrapper", n_dir, 20, 32, 5, seed=6)
    k, hop, A = T.case_hops(c)[1]
    x, X = _inputs(c, k, hop)
    raw = _call(c, hop, A, X)
    I, tabs = _engine_args(c, A, X)
    call = lambda I, tabs=tabs, **kw: engine.digraph_tlayer_bwd(I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"], *tabs,
                                                              edge_time=I["edge_time"], q_time=I["q_time"], n_dir=n_dir, **kw)
    gate, gh, gas = call(I)
    assert torch.equal(gate, raw[0]) and torch.equal(gh, raw[1]) and gas.shape == (hop.n_old, c.ap)
    want = raw[2] if n_dir == 1 else (raw[2].view(-1, 3, c.ap)[:, 0] + raw[2].view(-1, 3, c.ap)[:, 1]) + raw[2].view(-1, 3, c.ap)[:, 2]
    assert torch.equal(gas, want)
    f64 = T.backward(hop, *T.tables(x))
    np.testing.assert_allclose(gas.cpu().numpy(), T.group_directions(f64.grad_a_s_dir, n_dir), rtol=1e-4, atol=1e-5)
    again = call(I)
    assert all(torch.equal(a, b) for a, b in zip(again, (gate, gh, gas)))
    g1, h1, a1 = call(I, want_state=False)
    assert h1 is None and a1 is None and torch.equal(g1, raw[0])
    # the view the wrapper builds is the reference's
    key = engine.digraph_directed_rows(I["dst_ptr"], I["src_idx"], I["row_of_dst"], I["edge_time"], I["q_time"], n_dir)
    assert np.array_equal(key.cpu().numpy(), hop.hrow)
    V = T.directed_view(hop)
    ptr, ptr_h, edge_of, dst_of = engine.digraph_source_view(I["dst_ptr"], I["src_idx"], n_dir * hop.n_old, key=key)
    assert np.array_equal(ptr_h, V["src_ptr"]) and np.array_equal(edge_of.cpu().numpy(), V["edge_of"]) and np.array_equal(dst_of.cpu().numpy(), V["dst_of_edge"])
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    E0 = dict(I, dst_ptr=torch.zeros(hop.n_new + 1, dtype=torch.int32, device="cuda"), src_idx=none, rel=none, edge_time=none)
    g0, h0, a0 = call(E0)
    assert g0.numel() == 0 and h0.shape == X["hidden"].shape and not h0.any() and a0.shape == X["a_s"].shape and not a0.any()
    bads = [("src_idx", hop.n_old), ("rel", c.n_rela_rows), ("row_of_dst", X["a_q"].shape[0]), ("src_idx", -1), ("edge_time", -1)]
    if n_dir == 3:
        bads.append(("edge_time", c.n_tab_rows))
    for name, bad in bads:
        args = dict(I)
        args[name] = I[name].clone()
        args[name][0] = bad
        with pytest.raises(ValueError, match=name + " out of range"):
            call(args)
    with pytest.raises(ValueError, match="do not fit together"):
        call(I, tabs=tabs[:-1] + (X["grad_agg"][:-1].contiguous(),))
    with pytest.raises(ValueError, match="do not fit together"):
        call(I, tabs=(X["hidden"][:-1].contiguous(),) + tabs[1:])
    with pytest.raises(ValueError, match="do not fit together"):
        call(dict(I, edge_time=I["edge_time"][:-1].contiguous()))
    with pytest.raises(ValueError, match="n_dir must be 1 or 3"):
        engine.digraph_tlayer_bwd(I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"], *tabs, edge_time=I["edge_time"], q_time=I["q_time"],
                                  n_dir=2)


def test_no_edges_launches_nothing():
    c, hop, A = T.one_edge_hop(3)
    _, X = _inputs(c, 0, hop)
    empty = dict(dst_ptr=np.zeros(2, np.int32), src_idx=np.zeros(0, np.int32), rel=np.zeros(0, np.int32), row_of_dst=np.zeros(1, np.int32),
                 edge_time=np.zeros(0, np.int32))
    hop0 = T.timed_hop(empty, c.q_time, 3, hop.n_old, c.n_rela_rows, c.n_tab_rows)
    gate, gh, gas = _call(c, hop0, empty, X)
    assert gate.numel() == 0 and torch.isnan(gh).all() and torch.isnan(gas).all()     # success, and the outputs are left alone


def test_unsupported_attention_width_is_an_error_and_the_next_call_is_fine():
    from red_gnn_amd import _lib
    c = T.case("ap20", 3, 16, 32, 5, seed=7)
    k, hop, A = T.case_hops(c)[0]
    x, good = _inputs(c, k, hop)
    c.attn_dim = c.ap = 20
    _, X = _inputs(c, k, hop)
    with pytest.raises(_lib.NativeError, match="padded attention dim 20"):
        _call(c, hop, A, X)
    c.attn_dim, c.ap = 5, 8
    _check("after the error", c, _call(c, hop, A, good), T.backward(hop, *T.tables(x)))
