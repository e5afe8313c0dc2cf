"""rg_digraph_layer_fwd_gated and rg_digraph_layer_bwd_gated called on their own (-m gpu): one edge-list hop and its adjoint with a gate
on every edge's message, three replicas in one launch, against the fp64 per-edge reference of tests/digraph_gated_ref.py under
tests/layer_ref.py's error model as it stands, every gated term's magnitude scaled by |g| and one more rounding per term:

    |out - ref64| <= C_BOUND * (n + n0) * u * S + 1e-30            (digraph_gated_ref's docstring defines S, n, n0; C_BOUND = 1.6)

The cases are tests/digraph_bwd_ref.py's (row widths, attention widths, the hub sources, one edge), plus layer_ref's hub DESTINATIONS
for the forward's split; all with n_rep = 3, t = (0, 0.37, 1) and random gates that include an exact 0, an exact 1, a negative value and
a value above 1.  Every element of every output is checked, pad columns included; the outputs are pre-filled with NaN and two runs are
bit-equal.  Bit for bit: one replica at t = 1 with NULL gates, and gate_lo == gate_hi == 1, are the ungated kernels; replica k of the
three is the one-replica call with t[k]; the hubs alone are the hubs within the full call.
The kernels' worst ratios over these cases, as measured on an MI355X: 0.27 for agg (0.25 on the hub destinations), 0.06 for grad_gate,
0.14 for grad_hidden, 0.015 for grad_a_s (information only, the assertions use C_BOUND).  Wall time of this file there: 4.0 s (20
tests).
"""
import numpy as np
import pytest
import torch

from tests import digraph_bwd_ref as D
from tests import digraph_gated_ref as GR
from tests import layer_ref as lr

pytestmark = pytest.mark.gpu

N_REP = len(GR.T)


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _fwd(c, A, X, t, lo=None, hi=None, want_alpha=True, ap=None, n_rep=None, t_null=False):
    """The raw gated forward on numpy index arrays ``A`` and device inputs ``X`` (hidden / a_s stacked per replica): (agg pre-filled
    with NaN, alpha or None)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n_rep = len(t) if n_rep is None else n_rep
    n_dst, E, n_src = len(A["dst_ptr"]) - 1, len(A["src_idx"]), X["a_s"].shape[0] // max(len(t), 1)
    ap = c.ap if ap is None else ap
    I = {k: _dev(v, torch.int32) for k, v in A.items()}
    agg = _nan(len(t) * n_dst, c.ld)
    alpha = _nan(len(t) * E) if want_alpha else None
    nb = L.rg_digraph_layer_fwd_gated_scratch_bytes(p(A["dst_ptr"]), n_dst, c.ld, len(t)) if n_dst else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    t_d, lo_d, hi_d = _dev(t), _dev(lo), _dev(hi)                            # (held until the call has run)
    _lib.check(L.rg_digraph_layer_fwd_gated(n_rep, None if t_null else p(t_d), p(lo_d), p(hi_d), n_dst, E, p(I["dst_ptr"]),
                                            p(A["dst_ptr"]), p(I["src_idx"]), p(I["rel"]), p(I["row_of_dst"]), n_src, X["rela"].shape[0],
                                            X["a_q"].shape[0], p(X["hidden"]), p(X["rela"]), c.d, c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]),
                                            ap, p(X["w_alpha"]), p(X["b_alpha"]), c.attn_dim, p(agg), p(alpha), p(scratch), nb,
                                            _lib.stream_ptr()))
    torch.cuda.synchronize()
    return agg, alpha


def _bwd(c, A, V, X, t, lo=None, hi=None, want_state=True, n_rep=None, t_null=False):
    """The raw gated adjoint: (grad_gate, grad_hidden, grad_a_s) pre-filled with NaN (the last two None without ``want_state``)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n_rep = len(t) if n_rep is None else n_rep
    n_src, n_dst, E = len(V["src_ptr"]) - 1, len(A["dst_ptr"]) - 1, len(A["src_idx"])
    I = {k: _dev(v, torch.int32) for k, v in {**A, **V}.items()}
    gate = _nan(len(t) * E)
    gh, gas = (_nan(len(t) * n_src, c.ld), _nan(len(t) * n_src, c.ap)) if want_state else (None, None)
    nb = L.rg_digraph_layer_bwd_gated_scratch_bytes(p(V["src_ptr"]), n_src, c.ld, c.ap, len(t)) if n_src else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    t_d, lo_d, hi_d = _dev(t), _dev(lo), _dev(hi)                            # (held until the call has run)
    _lib.check(L.rg_digraph_layer_bwd_gated(n_rep, None if t_null else p(t_d), p(lo_d), p(hi_d), n_src, n_dst, E, p(I["src_ptr"]),
                                            p(V["src_ptr"]), p(I["edge_of"]), p(I["dst_of_edge"]), p(I["rel"]), p(I["row_of_dst"]),
                                            X["rela"].shape[0], X["a_q"].shape[0], p(X["hidden"]), p(X["rela"]), c.d, c.ld, p(X["a_s"]),
                                            p(X["a_r"]), p(X["a_q"]), c.ap, p(X["w_alpha"]), p(X["b_alpha"]), c.attn_dim, p(X["grad_agg"]),
                                            p(gate), p(gh), p(gas), p(scratch), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return gate, gh, gas


def _check(tag, c, names, got, f64):
    for name, t in zip(names, got):
        g = t.cpu().numpy().astype(np.float64)
        assert not np.isnan(g).any(), "%s: %d elements of %s were never written" % (tag, int(np.isnan(g).sum()), name)
        ref, n0 = getattr(f64, name), GR.n0_of(name, c.d, c.attn_dim)
        ok = np.abs(g - ref) <= lr.bound(f64.S[name], f64.n[name], n0, lr.C_BOUND)
        ratio = lr.worst_ratio(g, ref, f64.S[name], f64.n[name], n0)
        print("%s %s: worst ratio %.3g (allowed %.3g)" % (tag, name, ratio, lr.C_BOUND))
        assert ok.all(), "%s %s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g)" % (tag, name, int((~ok).sum()), ok.size,
                                                                                                       ratio, lr.C_BOUND)


def _replica_X(X, hop, j):
    rows = lambda a, n: a[j * n:(j + 1) * n].contiguous()
    return dict(X, hidden=rows(X["hidden"], hop.n_old), a_s=rows(X["a_s"], hop.n_old), grad_agg=rows(X["grad_agg"], hop.n_new))


def _ungated(c, A, V, X1):
    """rg_digraph_layer_fwd / rg_digraph_layer_bwd (both want-state forms) on one replica's inputs, through the sibling files' raw calls."""
    from tests.test_digraph_bwd_gpu import _call as bwd_call
    from tests.test_digraph_layer_gpu import _call as fwd_call
    return fwd_call(c, A, X1), bwd_call(c, A, V, X1), bwd_call(c, A, V, X1, want_state=False)


def _run_hop(tag, c, k, hop, A, forward_only=False):
    """One hop: three replicas against the reference, two runs, every replica against its own one-replica call, and gates of 1
    against the ungated kernels."""
    x = GR.replica_inputs(c, k, hop, N_REP)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    lo, hi = GR.gates(hop.E, k)
    V = D.source_view(A, hop.n_old)
    calls = [("fwd", GR.FWD_OUTPUTS, lambda XX, t, a, b, **kw: _fwd(c, A, XX, t, a, b, **kw), GR.forward)]
    if not forward_only:
        calls.append(("bwd", GR.BWD_OUTPUTS, lambda XX, t, a, b, **kw: _bwd(c, A, V, XX, t, a, b, **kw), GR.backward))
    out = {}
    for kind, names, call, ref in calls:
        got = call(X, GR.T, lo, hi)
        _check("%s %s" % (tag, kind), c, names, got, ref(hop, x, GR.T, lo, hi))
        if kind == "fwd":
            a64 = GR.forward(hop, x, GR.T, lo, hi).alpha
            a = got[1].cpu().numpy().astype(np.float64)
            assert not np.isnan(a).any() and np.abs(a - a64).max() <= 1e-5, tag + ": alpha_out"      # the gate does not enter alpha
            assert not got[0][:, c.d:].any(), tag + ": pad columns of agg"
        else:
            assert not got[2][:, c.attn_dim:].any(), tag + ": pad columns of grad_a_s"
        again = call(X, GR.T, lo, hi)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), "%s %s: two runs differ" % (tag, kind)
        for j in range(N_REP):                                                # replica j is the one-replica call with t[j]
            one = call(_replica_X(X, hop, j), GR.T[j:j + 1], lo, hi)
            for name, full, part in zip(names + ("alpha",), got, one):
                n = part.shape[0]
                assert torch.equal(full[j * n:(j + 1) * n], part), "%s %s: replica %d of %s differs from its own call" % (tag, kind, j, name)
        out[kind] = got
    # ---- gates of exactly 1: the ungated kernels, bit for bit, for NULL gates at t = 1 and for gate_lo == gate_hi == 1
    X1 = _replica_X(X, hop, 0)
    ones, t1, t_any = np.ones(hop.E, np.float32), np.ones(1, np.float32), np.array([0.37], np.float32)
    (agg_u, alpha_u), bwd_u, (gate_u, _, _) = _ungated(c, A, V, X1)
    for t, a, b in ((t1, None, None), (t_any, ones, ones), (t1, None, ones)):
        agg, alpha = _fwd(c, A, X1, t, a, b)
        assert torch.equal(agg, agg_u) and torch.equal(alpha, alpha_u), tag + ": the gated forward at gate 1 is not the ungated one"
        assert torch.equal(_fwd(c, A, X1, t, a, b, want_alpha=False)[0], agg_u)
        if not forward_only:
            got = _bwd(c, A, V, X1, t, a, b)
            assert all(torch.equal(p, q) for p, q in zip(got, bwd_u)), tag + ": the gated adjoint at gate 1 is not the ungated one"
            gate, none_h, none_as = _bwd(c, A, V, X1, t, a, b, want_state=False)
            assert none_h is None and none_as is None and torch.equal(gate, gate_u), tag + ": grad_gate without the state outputs"
    # ---- t = 0 on a baseline of 0: nothing passes, yet every gate has a gradient
    agg0, alpha0 = _fwd(c, A, X1, np.zeros(1, np.float32), None, hi)
    assert not agg0.any() and torch.equal(alpha0, alpha_u), tag + ": agg at gate 0"
    if not forward_only:
        gate0, gh0, gas0 = _bwd(c, A, V, X1, np.zeros(1, np.float32), None, hi)
        assert not gh0.any() and not gas0.any() and torch.equal(gate0, gate_u) and gate0.any(), tag + ": the adjoint at gate 0"
    return x, X, V, lo, hi, out


@pytest.mark.parametrize("d,ld", D.ROW_WIDTHS)
def test_row_widths(d, ld):
    c = D.row_width_case(d, ld)
    for k, hop, A in D.case_hops(c):
        _run_hop("%s hop %d" % (c.name, k + 1), c, k, hop, A)


@pytest.mark.parametrize("attn,ap", D.ATTENTION_WIDTHS)
def test_attention_widths(attn, ap):
    c = D.attention_case(attn, ap)
    for k, hop, A in D.case_hops(c):
        _run_hop("%s hop %d" % (c.name, k + 1), c, k, hop, A)


def test_one_edge():
    c, hop, A = D.one_edge_hop()
    _run_hop(c.name, c, 0, hop, A)


def test_hub_sources_the_hubs_alone_are_the_hubs_within_the_full_call():
    """Sources of 0, 1, 127, 128, 129, 256, 257 and 3000 out-edges among a thousand one-edge sources, three replicas: the adjoint's
    split per replica.  The hubs alone give bit for bit their rows and their edges' gate gradients within the full call."""
    from red_gnn_amd import engine
    c, hop, A = D.hub_hop()
    x, X, V, lo, hi, out = _run_hop(c.name, c, 0, hop, A)
    gate, gh, gas = out["bwd"]
    deg = np.diff(V["src_ptr"].astype(np.int64))
    assert engine.digraph_chunks(V["src_ptr"]) == (4, 2 + 2 + 3 + 24, 3000)
    for pick in (np.nonzero(deg > engine.DIGRAPH_CHUNK)[0], np.arange(0, len(deg), 3)):
        A2, V2, at = D.take_sources(A, V, pick)
        rows = np.concatenate([j * hop.n_old + pick for j in range(N_REP)])
        edges = torch.as_tensor(np.concatenate([j * hop.E + at for j in range(N_REP)])).cuda()
        X2 = dict(X, hidden=X["hidden"][rows].contiguous(), a_s=X["a_s"][rows].contiguous())
        g2, h2, as2 = _bwd(c, A2, V2, X2, GR.T, lo[at], hi[at])
        rows = torch.as_tensor(rows).cuda()
        assert torch.equal(g2, gate[edges]) and torch.equal(h2, gh[rows]) and torch.equal(as2, gas[rows]), \
            "a source's gradients depend on the rest of the call"


def test_hub_destinations_the_hubs_alone_are_the_hubs_within_the_full_call():
    """layer_ref's hub regime for the forward: destinations of 1 .. 3000 in-edges (3000: 24 chunks) among thousands of leaves, three
    replicas - the partial rows and the combine pass per replica."""
    from red_gnn_amd import engine
    c = lr.CASES["hubs"]()
    (k, hop, A), = D.case_hops(c)
    x, X, V, lo, hi, out = _run_hop(c.name, c, k, hop, A, forward_only=True)
    agg, alpha = out["fwd"]
    length = np.diff(A["dst_ptr"].astype(np.int64))
    n_hub, _, longest = engine.digraph_chunks(A["dst_ptr"])
    assert longest > 2 * engine.DIGRAPH_CHUNK and n_hub >= 4
    for pick in (np.nonzero(length > engine.DIGRAPH_CHUNK)[0], np.arange(0, len(length), 3)):
        at = np.concatenate([np.arange(A["dst_ptr"][o], A["dst_ptr"][o + 1]) for o in pick])
        ptr = np.zeros(len(pick) + 1, np.int32)
        ptr[1:] = np.cumsum(length[pick])
        sub = dict(dst_ptr=ptr, src_idx=A["src_idx"][at], rel=A["rel"][at], row_of_dst=A["row_of_dst"][pick])
        part, part_alpha = _fwd(c, sub, X, GR.T, lo[at], hi[at])
        rows = torch.as_tensor(np.concatenate([j * hop.n_new + pick for j in range(N_REP)])).cuda()
        edges = torch.as_tensor(np.concatenate([j * hop.E + at for j in range(N_REP)])).cuda()
        assert torch.equal(part, agg[rows]) and torch.equal(part_alpha, alpha[edges]), "a destination's row depends on the rest of the call"


def test_argument_errors_are_reported_and_nothing_is_launched():
    """n_rep < 1 or above 65535, replicas beyond int32, a NULL t, misaligned tables: non-zero with rg_last_error() set, the outputs still NaN."""
    from red_gnn_amd import _lib
    c, hop, A = D.hub_hop()
    x = GR.replica_inputs(c, 0, hop, 1)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    V = D.source_view(A, hop.n_old)
    t1 = np.ones(1, np.float32)
    off = lambda a: torch.cat([a.reshape(-1), a.new_zeros(4)])[1:1 + a.numel()].view(a.shape)      # the same shape, 4 bytes further on
    bad = [("need at least one replica", dict(n_rep=0), X), ("need at least one replica", dict(n_rep=-3), X),
           ("overflows int32", dict(n_rep=(1 << 31) // hop.E + 1), X), ("at most 65535", dict(n_rep=65536), X), ("NULL argument \\(t\\)", dict(t_null=True), X),
           ("16-B aligned", {}, dict(X, hidden=off(X["hidden"]))), ("16-B aligned", {}, dict(X, a_s=off(X["a_s"])))]
    for match, kw, XX in bad:
        for call in (lambda: _fwd(c, A, XX, t1, **kw), lambda: _bwd(c, A, V, XX, t1, **kw)):
            with pytest.raises(_lib.NativeError, match=match):
                call()
    # (the raw helpers pre-fill with NaN; a failed call must leave that as it is: checked through the library directly)
    L, p = _lib.lib(), _lib.ptr
    I = {k: _dev(v, torch.int32) for k, v in {**A, **V}.items()}
    agg, gate = _nan(hop.n_new, c.ld), _nan(hop.E)
    t_d = _dev(t1)
    rc = L.rg_digraph_layer_fwd_gated(0, p(t_d), None, None, hop.n_new, hop.E, p(I["dst_ptr"]), p(A["dst_ptr"]), p(I["src_idx"]),
                                      p(I["rel"]), p(I["row_of_dst"]), hop.n_old, X["rela"].shape[0], X["a_q"].shape[0], p(X["hidden"]),
                                      p(X["rela"]), c.d, c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), c.ap, p(X["w_alpha"]), p(X["b_alpha"]),
                                      c.attn_dim, p(agg), None, None, 0, _lib.stream_ptr())
    assert rc != 0 and b"n_rep" in L.rg_last_error()
    rc = L.rg_digraph_layer_bwd_gated(1, None, None, None, hop.n_old, hop.n_new, hop.E, p(I["src_ptr"]), p(V["src_ptr"]), p(I["edge_of"]),
                                      p(I["dst_of_edge"]), p(I["rel"]), p(I["row_of_dst"]), X["rela"].shape[0], X["a_q"].shape[0],
                                      p(X["hidden"]), p(X["rela"]), c.d, c.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), c.ap, p(X["w_alpha"]),
                                      p(X["b_alpha"]), c.attn_dim, p(X["grad_agg"]), p(gate), None, None, None, 0, _lib.stream_ptr())
    assert rc != 0 and b"NULL argument (t)" in L.rg_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(agg).all() and torch.isnan(gate).all()
    # indices outside their tables are clamped, never followed: the call succeeds and writes every row
    wild = dict(A, src_idx=A["src_idx"].copy(), rel=A["rel"].copy())
    wild["src_idx"][::7], wild["rel"][::5] = 1 << 30, -5
    agg, _ = _fwd(c, wild, X, t1)
    assert bool(torch.isfinite(agg).all())


def test_engine_wrappers_check_and_match():
    """engine.digraph_layer_fwd_gated / digraph_layer_bwd_gated: the raw calls' bits (with a source view handed over or built), and the
    ValueErrors of their ungated siblings plus those of t and the gates."""
    from red_gnn_amd import engine
    c = D.case("wrapper", 20, 32, 5, seed=6)
    k, hop, A = D.case_hops(c)[1]
    x = GR.replica_inputs(c, k, hop, N_REP)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    lo, hi = GR.gates(hop.E, k)
    V = D.source_view(A, hop.n_old)
    raw_f, raw_b = _fwd(c, A, X, GR.T, lo, hi), _bwd(c, A, V, X, GR.T, lo, hi)
    I = {kk: _dev(v, torch.int32) for kk, v in A.items()}
    idx = (I["dst_ptr"], I["src_idx"], I["rel"], I["row_of_dst"])
    tabs = (X["hidden"], X["rela"], c.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], c.attn_dim)
    t, glo, ghi = _dev(GR.T), _dev(lo), _dev(hi)
    got = engine.digraph_layer_fwd_gated(*idx, *tabs, t, glo, ghi)
    assert all(torch.equal(a, b) for a, b in zip(got, raw_f))
    got = engine.digraph_layer_bwd_gated(*idx, *tabs, X["grad_agg"], t, glo, ghi)
    assert all(torch.equal(a, b) for a, b in zip(got, raw_b))
    view = engine.digraph_source_view(I["dst_ptr"], I["src_idx"], hop.n_old)
    gate, gh, gas = engine.digraph_layer_bwd_gated(*idx, *tabs, X["grad_agg"], t, glo, ghi, want_state=False, view=view, check_index=False)
    assert gh is None and gas is None and torch.equal(gate, raw_b[0])
    with pytest.raises(ValueError, match="t must be a float32 vector"):
        engine.digraph_layer_fwd_gated(*idx, *tabs, t[:0])
    with pytest.raises(ValueError, match="gate_lo must be float32"):
        engine.digraph_layer_fwd_gated(*idx, *tabs, t, glo[:-1], ghi)
    with pytest.raises(ValueError, match="gate_hi must be float32"):
        engine.digraph_layer_bwd_gated(*idx, *tabs, X["grad_agg"], t, glo, ghi.double())
    with pytest.raises(ValueError, match="whole number of rows"):
        engine.digraph_layer_fwd_gated(*idx, *tabs, torch.ones(X["a_s"].shape[0] + 1, device="cuda"), glo, ghi)
    bad = I["src_idx"].clone()
    bad[0] = hop.n_old                                                        # replica 1's row 0: outside the hop's own sources
    with pytest.raises(ValueError, match="src_idx out of range"):
        engine.digraph_layer_fwd_gated(I["dst_ptr"], bad, I["rel"], I["row_of_dst"], *tabs, t, glo, ghi)
    with pytest.raises(ValueError, match="do not fit together"):
        engine.digraph_layer_bwd_gated(*idx, *tabs, X["grad_agg"][:-1].contiguous(), t, glo, ghi)
