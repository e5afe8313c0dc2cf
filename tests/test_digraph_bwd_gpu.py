"""rg_digraph_layer_bwd called on its own (-m gpu): the adjoint of one edge-list hop with respect to the gates, the source states and
their attention projection, against the fp64 per-edge reference of tests/digraph_bwd_ref.py under tests/layer_ref.py's error model
unchanged:

    |out - ref64| <= C_BOUND * (n + n0) * u * S + 1e-30            (layer_ref's docstring defines S, n, n0; C_BOUND = 1.6; grad_gate's S, n
                                                                    and n0: digraph_bwd_ref's docstring)

The edge lists are the CPU oracle's hops (layer_ref.hops) re-ordered by destination, as tests/test_digraph_layer_gpu.py hands them to
the forward, plus a hand-built hub list.  Every element of every output is checked, pad columns included; the outputs are pre-filled
with NaN (every row must be written) and two runs are bit-equal.
The kernel's worst ratios over these cases, as measured on an MI355X: 0.06 for grad_gate, 0.14 for grad_hidden, 0.013 for grad_a_s
(information only, the assertions use C_BOUND).  Wall time of this file there: 3.8 s (20 tests).
"""
import numpy as np
import pytest
import torch

from tests import digraph_bwd_ref as D
from tests import layer_ref as lr

pytestmark = pytest.mark.gpu


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _inputs(c, k, hop):
    x = lr.inputs(c, k, hop)
    return x, {kk: _dev(v) for kk, v in x.items() if v is not None}


def _call(c, A, V, X, ap=None, attn=None, want_state=True):
    """The raw entry point on numpy index arrays ``A`` (the forward's) and ``V`` (the source view) and device inputs ``X``:
    (grad_gate, grad_hidden, grad_a_s) pre-filled with NaN (the last two None without ``want_state``)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n_src, n_dst, E = len(V["src_ptr"]) - 1, len(A["dst_ptr"]) - 1, len(A["src_idx"])
    ap = c.ap if ap is None else ap
    I = {k: _dev(v, torch.int32) for k, v in {**A, **V}.items()}
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    gate, gh, gas = nan(E), nan(n_src, c.ld) if want_state else None, nan(n_src, ap) if want_state else None
    nb = L.rg_digraph_layer_bwd_scratch_bytes(p(V["src_ptr"]), n_src, c.ld, ap) if n_src else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    _lib.check(L.rg_digraph_layer_bwd(n_src, n_dst, E, p(I["src_ptr"]), p(V["src_ptr"]), p(I["edge_of"]), p(I["dst_of_edge"]), p(I["rel"]),
                                      p(I["row_of_dst"]), X["rela"].shape[0], X["a_q"].shape[0], p(X["hidden"]), p(X["rela"]), c.d, c.ld,
                                      p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), ap, p(X["w_alpha"]), p(X["b_alpha"]),
                                      c.attn_dim if attn is None else attn, p(X["grad_agg"]), p(gate), p(gh), p(gas), p(scratch), nb,
                                      _lib.stream_ptr()))
    torch.cuda.synchronize()
    return gate, gh, gas


def _check(tag, c, got, f64):
    for name, t in zip(D.OUTPUTS, got):
        g = t.cpu().numpy().astype(np.float64)
        assert not np.isnan(g).any(), "%s: %d elements of %s were never written" % (tag, int(np.isnan(g).sum()), name)
        ref, n0 = getattr(f64, name), D.n0_of(name, c.d, c.attn_dim)
        ok = np.abs(g - ref) <= lr.bound(f64.S[name], f64.n[name], n0, lr.C_BOUND)
        ratio = lr.worst_ratio(g, ref, f64.S[name], f64.n[name], n0)
        print("%s %s: worst ratio %.3g (allowed %.3g)" % (tag, name, ratio, lr.C_BOUND))
        assert ok.all(), "%s %s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g)" % (tag, name, int((~ok).sum()), ok.size,
                                                                                                       ratio, lr.C_BOUND)
    assert not got[2][:, c.attn_dim:].any(), tag + ": pad columns of grad_a_s"


def _run_hop(tag, c, k, hop, A):
    """One hop: the kernel against the reference, two runs bit for bit, and the gate gradients alone (NULL state outputs)."""
    x, X = _inputs(c, k, hop)
    V = D.source_view(A, hop.n_old)
    got = _call(c, A, V, X)
    _check(tag, c, got, D.backward(hop, *D.tables(x)))
    again = _call(c, A, V, X)
    assert all(torch.equal(a, b) for a, b in zip(got, again)), tag + ": two runs differ"
    gate, none_h, none_as = _call(c, A, V, X, want_state=False)
    assert none_h is None and none_as is None and torch.equal(gate, got[0]), tag + ": grad_gate without the state outputs"
    if c.d < c.ld:                  # layer_ref's grad_agg fills its pad columns; with them zero, those of grad_hidden are zero
        G = X["grad_agg"].clone()
        G[:, c.d:] = 0
        padded = _call(c, A, V, dict(X, grad_agg=G))
        assert not padded[1][:, c.d:].any() and torch.equal(padded[1][:, :c.d], got[1][:, :c.d]), tag + ": pad columns of grad_hidden"
    return V, X, got


def _run_case(c):
    for k, hop, A in D.case_hops(c):
        _run_hop("%s hop %d" % (c.name, k + 1), c, k, hop, A)


@pytest.mark.parametrize("d,ld", D.ROW_WIDTHS)
def test_row_widths(d, ld):
    _run_case(D.row_width_case(d, ld))


@pytest.mark.parametrize("attn,ap", D.ATTENTION_WIDTHS)
def test_attention_widths(attn, ap):
    _run_case(D.attention_case(attn, ap))


def test_hub_sources_next_to_many_one_edge_sources():
    """Sources of 0, 1, 127, 128, 129, 256, 257 and 3000 out-edges (3000: 24 chunks; 128: the longest that is not cut) among a thousand
    one-edge sources.  A source's rows and its edges' gate gradients do not depend on what else the call carries: the hubs alone, and
    every third source, give bit for bit those of the full call."""
    from red_gnn_amd import engine
    c, hop, A = D.hub_hop()
    V, X, (gate, gh, gas) = _run_hop(c.name, c, 0, hop, A)
    deg = np.diff(V["src_ptr"].astype(np.int64))
    n_hub, n_chunks, longest = engine.digraph_chunks(V["src_ptr"])
    assert (n_hub, n_chunks, longest) == (4, 2 + 2 + 3 + 24, 3000) and (deg == 1).sum() > 1000 and (deg == engine.DIGRAPH_CHUNK).any()
    assert not gh[0].any() and not gas[0].any()                                       # the source without edges: zero rows
    for pick in (np.nonzero(deg > engine.DIGRAPH_CHUNK)[0], np.arange(0, len(deg), 3), np.array([int(deg.argmax())])):
        A2, V2, at = D.take_sources(A, V, pick)
        X2 = dict(X, hidden=X["hidden"][pick].contiguous(), a_s=X["a_s"][pick].contiguous())
        g2, h2, as2 = _call(c, A2, V2, X2)
        rows = torch.as_tensor(pick).cuda()
        assert torch.equal(g2, gate[torch.as_tensor(at).cuda()]) and torch.equal(h2, gh[rows]) and torch.equal(as2, gas[rows]), \
            "a source's gradients depend on the rest of the call"


def test_one_source_with_one_edge():
    c, hop, A = D.one_edge_hop()
    x, X = _inputs(c, 0, hop)
    V = D.source_view(A, hop.n_old)
    got = _call(c, A, V, X)
    _check("one edge", c, got, D.backward(hop, *D.tables(x)))
    assert got[0].shape == (1,) and float(got[0][0]) != 0.0 and not got[1][:3].any() and got[1][3].any()


def test_engine_wrapper_checks_and_matches():
    """engine.digraph_layer_bwd builds the source view itself: the raw call's bits, None state outputs on request, E == 0, and
    ValueError for indices outside their tables."""
    from red_gnn_amd import engine
    c = D.case("wrapper", 20, 32, 5, seed=6)
    k, hop, A = D.case_hops(c)[1]
    x, X = _inputs(c, k, hop)
    raw = _call(c, A, D.source_view(A, hop.n_old), X)
    I = {kk: _dev(v, torch.int32) for kk, v in A.items()}
    tabs = (X["hidden"], X["rela"], c.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], c.attn_dim, X["grad_agg"])
    got = engine.digraph_layer_bwd(I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"], *tabs)
    assert all(torch.equal(a, b) for a, b in zip(got, raw))
    gate, gh, gas = engine.digraph_layer_bwd(I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"], *tabs, want_state=False)
    assert gh is None and gas is None and torch.equal(gate, raw[0])
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    g0, h0, a0 = engine.digraph_layer_bwd(torch.zeros(hop.n_new + 1, dtype=torch.int32, device="cuda"), none, none, I["row_of_dst"], *tabs)
    assert g0.numel() == 0 and h0.shape == X["hidden"].shape and not h0.any() and not a0.any()
    for name, bad in (("src_idx", X["hidden"].shape[0]), ("rel", X["rela"].shape[0]), ("row_of_dst", X["a_q"].shape[0]), ("src_idx", -1)):
        args = dict(I)
        args[name] = I[name].clone()
        args[name][0] = bad
        with pytest.raises(ValueError, match=name + " out of range"):
            engine.digraph_layer_bwd(args["dst_ptr"], args["src_idx"], args["rel"], args["row_of_dst"], *tabs)
    with pytest.raises(ValueError, match="do not fit together"):
        engine.digraph_layer_bwd(I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"], *tabs[:-1], X["grad_agg"][:-1].contiguous())


def test_no_edges_launches_nothing():
    from red_gnn_amd import _lib
    c, hop, A = D.one_edge_hop()
    _, X = _inputs(c, 0, hop)
    empty = dict(dst_ptr=np.zeros(2, np.int32), src_idx=np.zeros(0, np.int32), rel=np.zeros(0, np.int32), row_of_dst=np.zeros(1, np.int32))
    gate, gh, gas = _call(c, empty, D.source_view(empty, hop.n_old), X)
    assert gate.numel() == 0 and torch.isnan(gh).all() and torch.isnan(gas).all()     # success, and the outputs are left alone
    assert _lib.lib().rg_digraph_layer_bwd(*([0, 0, 0] + [None] * 6 + [0, 0, None, None, 16, 16, None, None, None, 4, None, None, 3] +
                                             [None] * 5 + [0, None])) == 0


def test_unsupported_attention_width_is_an_error_and_the_next_call_is_fine():
    from red_gnn_amd import _lib
    c = D.case("ap20", 16, 32, 5, seed=7)
    k, hop, A = D.case_hops(c)[0]
    x, good = _inputs(c, k, hop)
    V = D.source_view(A, hop.n_old)
    c.attn_dim = c.ap = 20
    _, X = _inputs(c, k, hop)
    with pytest.raises(_lib.NativeError, match="padded attention dim 20"):
        _call(c, A, V, X)
    c.attn_dim, c.ap = 5, 8
    _check("after the error", c, _call(c, A, V, good), D.backward(hop, *D.tables(x)))
