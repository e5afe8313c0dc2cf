"""rg_digraph_layer_fwd_gates and rg_digraph_layer_bwd_gates called on their own (-m gpu): the gated edge-list hop and its adjoint with
a gate per (replica, edge).  What defines them is a condition on bits: replica k's outputs - agg, alpha_out, grad_gate, grad_hidden,
grad_a_s - are those of an n_rep = 1 call of the existing _gated entry point with gate_lo == gate_hi == gate[k] and t = 1, whatever
else the call carries.  (The _gated calls themselves are held to the fp64 reference by tests/test_digraph_gated_gpu.py.)

Over every hop of tests/digraph_gated_ref.all_hops() - every row width, attention width, the hub sources of 0, 1, 127, 128, 129, 256,
257 and 3000 out-edges and the one-edge hop - with n_rep 1 and 3 and digraph_gated_ref.gates' values (an exact 0, an exact 1, a
negative value, a value above 1): np.array_equal on every output of both calls, with and without the state outputs, the replicas
permuted, two runs; then the argument errors and the engine wrappers.  Wall time of this file on an MI355X: 3.4 s (66 tests)."""
import numpy as np
import pytest
import torch

from tests import digraph_bwd_ref as D
from tests import digraph_gated_ref as GR
from tests.test_digraph_gated_gpu import _bwd, _dev, _fwd, _nan, _replica_X

pytestmark = pytest.mark.gpu

ONE = np.ones(1, np.float32)


def _fwd_gates(c, A, X, gate, want_alpha=True, n_rep=None, gate_null=False):
    """The raw call on numpy index arrays ``A``, device inputs ``X`` (stacked per replica) and ``gate`` numpy [n_rep, E]: (agg pre-filled
    with NaN, alpha or None)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    R = gate.shape[0]
    n_rep = R if n_rep is None else n_rep
    n_dst, E, n_src = len(A["dst_ptr"]) - 1, len(A["src_idx"]), X["a_s"].shape[0] // R
    I = {k: _dev(v, torch.int32) for k, v in A.items()}
    agg = _nan(R * n_dst, c.ld)
    alpha = _nan(R * E) if want_alpha else None
    nb = L.rg_digraph_layer_fwd_gated_scratch_bytes(p(A["dst_ptr"]), n_dst, c.ld, R) if n_dst else 0       # the _gated function serves
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    g_d = _dev(gate)
    _lib.check(L.rg_digraph_layer_fwd_gates(n_rep, None if gate_null else p(g_d), n_dst, E, p(I["dst_ptr"]), p(A["dst_ptr"]),
                                            p(I["src_idx"]), p(I["rel"]), p(I["row_of_dst"]), n_src, X["rela"].shape[0], X["a_q"].shape[0],
                                            p(X["hidden"]), p(X["rela"]), c.d, c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), c.ap,
                                            p(X["w_alpha"]), p(X["b_alpha"]), c.attn_dim, p(agg), p(alpha), p(scratch), nb,
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    return agg, alpha


def _bwd_gates(c, A, V, X, gate, want_state=True, n_rep=None, gate_null=False):
    """The raw adjoint: (grad_gate, grad_hidden, grad_a_s) pre-filled with NaN (the last two None without ``want_state``)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    R = gate.shape[0]
    n_rep = R if n_rep is None else n_rep
    n_src, n_dst, E = len(V["src_ptr"]) - 1, len(A["dst_ptr"]) - 1, len(A["src_idx"])
    I = {k: _dev(v, torch.int32) for k, v in {**A, **V}.items()}
    gg = _nan(R * E)
    gh, gas = (_nan(R * n_src, c.ld), _nan(R * n_src, c.ap)) if want_state else (None, None)
    nb = L.rg_digraph_layer_bwd_gated_scratch_bytes(p(V["src_ptr"]), n_src, c.ld, c.ap, R) if n_src else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    g_d = _dev(gate)
    _lib.check(L.rg_digraph_layer_bwd_gates(n_rep, None if gate_null else p(g_d), n_src, n_dst, E, p(I["src_ptr"]), p(V["src_ptr"]),
                                            p(I["edge_of"]), p(I["dst_of_edge"]), p(I["rel"]), p(I["row_of_dst"]), X["rela"].shape[0],
                                            X["a_q"].shape[0], p(X["hidden"]), p(X["rela"]), c.d, c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]),
                                            c.ap, p(X["w_alpha"]), p(X["b_alpha"]), c.attn_dim, p(X["grad_agg"]), p(gg), p(gh), p(gas),
                                            p(scratch), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return gg, gh, gas


def _gate_rows(E, k, n_rep):
    """float32 [n_rep, E]: digraph_gated_ref.gates' two arrays, then one more of another seed."""
    lo, hi = GR.gates(E, k)
    return np.stack([lo, hi, GR.gates(E, k + 50)[0]][:n_rep]).astype(np.float32)


def _same(tag, name, full, part, j):
    n = part.shape[0]
    got, want = full[j * n:(j + 1) * n].cpu().numpy(), part.cpu().numpy()
    assert not np.isnan(got).any(), "%s: %s of replica %d was not written everywhere" % (tag, name, j)
    assert np.array_equal(got, want), "%s: %s of replica %d differs from the one-replica _gated call in %d of %d elements" % (
        tag, name, j, int((got != want).sum()), got.size)


def _stack_X(X, hop, order):
    """The replicas ``order`` of X's stacked arrays, stacked again."""
    parts = [_replica_X(X, hop, j) for j in order]
    return dict(X, **{name: torch.cat([p[name] for p in parts], 0).contiguous() for name in ("hidden", "a_s", "grad_agg")})


def _run_hop(tag, c, k, hop, A, n_rep):
    x = GR.replica_inputs(c, k, hop, n_rep)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    V = D.source_view(A, hop.n_old)
    gate = _gate_rows(hop.E, k, n_rep)
    assert (gate == 0).any() and (gate == 1).any() and (gate < 0).any() and (gate > 1).any() or hop.E < 4
    fwd, bwd, bwd_ns = _fwd_gates(c, A, X, gate), _bwd_gates(c, A, V, X, gate), _bwd_gates(c, A, V, X, gate, want_state=False)
    fwd_na = _fwd_gates(c, A, X, gate, want_alpha=False)
    assert bwd_ns[1] is None and bwd_ns[2] is None and fwd_na[1] is None
    for j in range(n_rep):                                                    # the condition that defines the calls
        Xj = _replica_X(X, hop, j)
        for name, full, part in zip(("agg", "alpha"), fwd, _fwd(c, A, Xj, ONE, gate[j], gate[j])):
            _same(tag, name, full, part, j)
        _same(tag, "agg without alpha_out", fwd_na[0], _fwd(c, A, Xj, ONE, gate[j], gate[j], want_alpha=False)[0], j)
        for name, full, part in zip(GR.BWD_OUTPUTS, bwd, _bwd(c, A, V, Xj, ONE, gate[j], gate[j])):
            _same(tag, name, full, part, j)
        _same(tag, "grad_gate without the state outputs", bwd_ns[0], _bwd(c, A, V, Xj, ONE, gate[j], gate[j], want_state=False)[0], j)
    again = _fwd_gates(c, A, X, gate) + _bwd_gates(c, A, V, X, gate)
    assert all(torch.equal(a, b) for a, b in zip(again, fwd + bwd)), tag + ": two runs differ"
    if n_rep > 1:                                                             # the replicas permuted: the outputs permuted
        order = list(range(1, n_rep)) + [0]
        Xp, gp = _stack_X(X, hop, order), gate[order]
        for name, full, perm in zip(("agg", "alpha") + GR.BWD_OUTPUTS, fwd + bwd, _fwd_gates(c, A, Xp, gp) + _bwd_gates(c, A, V, Xp, gp)):
            n = full.shape[0] // n_rep
            want = torch.cat([full[j * n:(j + 1) * n] for j in order], 0)
            assert torch.equal(perm, want), "%s: %s of the permuted call is not the permuted %s" % (tag, name, name)


HOPS = GR.all_hops()


@pytest.mark.parametrize("n_rep", [1, 3])
@pytest.mark.parametrize("i", range(len(HOPS)), ids=[h[0].replace(" ", "_") for h in HOPS])
def test_every_replica_has_the_bits_of_its_one_replica_gated_call(i, n_rep):
    tag, c, k, hop, A = HOPS[i]
    _run_hop("%s n_rep=%d" % (tag, n_rep), c, k, hop, A, n_rep)


def test_argument_errors_are_reported_and_nothing_is_launched():
    from red_gnn_amd import _lib
    c, hop, A = D.hub_hop()
    x = GR.replica_inputs(c, 0, hop, 1)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    V = D.source_view(A, hop.n_old)
    gate = _gate_rows(hop.E, 0, 1)
    off = lambda a: torch.cat([a.reshape(-1), a.new_zeros(4)])[1:1 + a.numel()].view(a.shape)      # the same shape, 4 bytes further on
    bad = [("need at least one replica", dict(n_rep=0), X), ("need at least one replica", dict(n_rep=-3), X),
           ("overflows int32", dict(n_rep=(1 << 31) // hop.E + 1), X), ("at most 65535", dict(n_rep=65536), X),
           ("NULL argument \\(gate\\)", dict(gate_null=True), X), ("16-B aligned", {}, dict(X, hidden=off(X["hidden"])))]
    for match, kw, XX in bad:
        for call in (lambda: _fwd_gates(c, A, XX, gate, **kw), lambda: _bwd_gates(c, A, V, XX, gate, **kw)):
            with pytest.raises(_lib.NativeError, match=match):
                call()
    # a failed call leaves the outputs as they were: through the library directly, the outputs pre-filled with NaN
    L, p = _lib.lib(), _lib.ptr
    I = {k: _dev(v, torch.int32) for k, v in {**A, **V}.items()}
    agg, gg = _nan(hop.n_new, c.ld), _nan(hop.E)
    rc = L.rg_digraph_layer_fwd_gates(1, None, hop.n_new, hop.E, p(I["dst_ptr"]), p(A["dst_ptr"]), p(I["src_idx"]), p(I["rel"]),
                                      p(I["row_of_dst"]), hop.n_old, X["rela"].shape[0], X["a_q"].shape[0], p(X["hidden"]), p(X["rela"]), c.d,
                                      c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), c.ap, p(X["w_alpha"]), p(X["b_alpha"]), c.attn_dim, p(agg),
                                      None, None, 0, _lib.stream_ptr())
    assert rc != 0 and b"NULL argument (gate)" in L.rg_last_error()
    g_d = _dev(gate)
    rc = L.rg_digraph_layer_bwd_gates(0, p(g_d), hop.n_old, hop.n_new, hop.E, p(I["src_ptr"]), p(V["src_ptr"]), p(I["edge_of"]),
                                      p(I["dst_of_edge"]), p(I["rel"]), p(I["row_of_dst"]), X["rela"].shape[0], X["a_q"].shape[0],
                                      p(X["hidden"]), p(X["rela"]), c.d, c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), c.ap, p(X["w_alpha"]),
                                      p(X["b_alpha"]), c.attn_dim, p(X["grad_agg"]), p(gg), None, None, None, 0, _lib.stream_ptr())
    assert rc != 0 and b"n_rep" in L.rg_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(agg).all() and torch.isnan(gg).all()


def test_engine_wrappers_check_and_match():
    """engine.digraph_layer_fwd_gates / digraph_layer_bwd_gates: the raw calls' bits, and their ValueErrors."""
    from red_gnn_amd import engine
    c = D.case("wrapper", 20, 32, 5, seed=6)
    k, hop, A = D.case_hops(c)[1]
    x = GR.replica_inputs(c, k, hop, 3)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    V = D.source_view(A, hop.n_old)
    gate = _gate_rows(hop.E, k, 3)
    raw_f, raw_b = _fwd_gates(c, A, X, gate), _bwd_gates(c, A, V, X, gate)
    I = {kk: _dev(v, torch.int32) for kk, v in A.items()}
    idx = (I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"])
    tabs = (X["hidden"], X["rela"], c.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], c.attn_dim)
    g = _dev(gate)
    assert all(torch.equal(a, b) for a, b in zip(engine.digraph_layer_fwd_gates(*idx, *tabs, g), raw_f))
    assert all(torch.equal(a, b) for a, b in zip(engine.digraph_layer_bwd_gates(*idx, *tabs, X["grad_agg"], g), raw_b))
    view = engine.digraph_source_view(I["dst_ptr"], I["src_idx"], hop.n_old)
    gg, gh, gas = engine.digraph_layer_bwd_gates(*idx, *tabs, X["grad_agg"], g, want_state=False, view=view, check_index=False)
    assert gh is None and gas is None and torch.equal(gg, raw_b[0])
    for wrong in (g[:, :-1].contiguous(), g.reshape(-1), g.double(), g[:0]):
        with pytest.raises(ValueError, match="gate must be float32 \\[n_rep, %d\\]" % hop.E):
            engine.digraph_layer_fwd_gates(*idx, *tabs, wrong)
        with pytest.raises(ValueError, match="gate must be float32 \\[n_rep, %d\\]" % hop.E):
            engine.digraph_layer_bwd_gates(*idx, *tabs, X["grad_agg"], wrong)
    with pytest.raises(ValueError, match="whole number of rows"):
        engine.digraph_layer_fwd_gates(*idx, *tabs, torch.ones((X["a_s"].shape[0] + 1, hop.E), device="cuda"))
