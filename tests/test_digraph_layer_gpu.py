"""rg_digraph_layer_fwd called on its own (-m gpu): one message-passing layer over an explicit, destination-segmented edge list against
the fp64 per-edge reference of tests/layer_ref.py, under that file's error model unchanged:

    |agg - ref64| <= C_BOUND * (n + n0) * u * S + 1e-30                (layer_ref's docstring defines S, n, n0; C_BOUND = 1.6)

The edge lists are the CPU oracle's hops (layer_ref.hops) re-ordered by destination, so the reference sums every destination in the
order the kernel is handed.  Every element is checked, pad columns included; agg is pre-filled with NaN (every row must be written).
The kernel's worst ratio over these cases, as measured on an MI355X: 0.2 (the hub case; information only, the assertion uses C_BOUND).
Wall time of this file there: 3.9 s (22 tests).
"""
import types

import numpy as np
import pytest
import torch

from tests import layer_ref as lr

pytestmark = pytest.mark.gpu

KEYS = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _by_destination(edges, n_old, n_new):
    """The oracle's hop edges (batch, head, rel, tail, old_idx, new_idx) in destination order (stable: fact-row order inside one), as a
    layer_ref hop plus the kernel's arrays (dst_ptr, src_idx, rel, row_of_dst) in numpy."""
    e = np.asarray(edges, np.int64)
    e = e[np.argsort(e[:, 5], kind="stable")]
    hop = lr.static_hop(e, n_old, n_new)
    ptr = np.zeros(n_new + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(e[:, 5], minlength=n_new))
    row_of = np.zeros(n_new, np.int64)
    row_of[e[:, 5]] = e[:, 0]
    return hop, dict(dst_ptr=ptr.astype(np.int32), src_idx=e[:, 4].astype(np.int32), rel=e[:, 2].astype(np.int32),
                     row_of_dst=row_of.astype(np.int32))


def _call(case, A, X, ap=None, attn=None, want_alpha=True):
    """The raw entry point on numpy index arrays ``A`` and device inputs ``X``: (agg pre-filled with NaN, alpha or None)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n_dst, E = len(A["dst_ptr"]) - 1, len(A["src_idx"])
    D = {k: _dev(v, torch.int32) for k, v in A.items()}
    agg = torch.full((n_dst, case.ld), float("nan"), dtype=torch.float32, device="cuda")
    alpha = torch.full((E,), float("nan"), dtype=torch.float32, device="cuda") if want_alpha else None
    nb = L.rg_digraph_layer_fwd_scratch_bytes(p(A["dst_ptr"]), n_dst, case.ld) if n_dst else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    _lib.check(L.rg_digraph_layer_fwd(n_dst, E, p(D["dst_ptr"]), p(A["dst_ptr"]), p(D["src_idx"]), p(D["rel"]), p(D["row_of_dst"]),
                                      X["hidden"].shape[0], X["rela"].shape[0], X["a_q"].shape[0], p(X["hidden"]), p(X["rela"]), case.d,
                                      case.ld, p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), case.ap if ap is None else ap, p(X["w_alpha"]),
                                      p(X["b_alpha"]), case.attn_dim if attn is None else attn, p(agg), p(alpha), p(scratch), nb,
                                      _lib.stream_ptr()))
    torch.cuda.synchronize()
    return agg, alpha


def _check(tag, case, agg, f64):
    got = agg.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), "%s: %d elements of agg were never written" % (tag, int(np.isnan(got).sum()))
    n0 = lr.n0_of("agg", case.d, case.attn_dim)
    ok = np.abs(got - f64.agg) <= lr.bound(f64.S["agg"], f64.n["agg"], n0, lr.C_BOUND)
    ratio = lr.worst_ratio(got, f64.agg, f64.S["agg"], f64.n["agg"], n0)
    print("%s: worst ratio %.3g (allowed %.3g)" % (tag, ratio, lr.C_BOUND))
    assert ok.all(), "%s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g)" % (tag, int((~ok).sum()), ok.size, ratio,
                                                                                                lr.C_BOUND)
    assert not agg[:, case.d:].any(), tag + ": pad columns of agg"


def _run_case(case):
    """Every hop of the case: the kernel against the reference, alpha against the reference's, two runs bit for bit."""
    for k, (old, new, edges, _) in enumerate(lr.hops(case)):
        tag = "%s hop %d" % (case.name, k + 1)
        hop, A = _by_destination(edges, len(old), len(new))
        x = lr.inputs(case, k, hop)
        X = {kk: _dev(v) for kk, v in x.items() if v is not None}
        f64 = lr.forward(hop, *(x[kk] for kk in KEYS))
        agg, alpha = _call(case, A, X)
        _check(tag, case, agg, f64)
        a = alpha.cpu().numpy().astype(np.float64)
        assert not np.isnan(a).any() and np.abs(a - f64.alpha).max() <= 1e-5, tag + ": alpha_out"
        again, alpha2 = _call(case, A, X)
        assert torch.equal(again, agg) and torch.equal(alpha2, alpha), tag + ": two runs differ"
        none, _ = _call(case, A, X, want_alpha=False)                         # alpha_out = NULL is accepted and changes nothing
        assert torch.equal(none, agg), tag
    return hop, A, x, X, agg


def _case(name, d, ld, attn, ap=None, seed=0, **kw):
    c = lr._case(name, seed=seed, d=d, ld=ld, attn_dim=attn, B=5, **kw)
    if ap is not None:
        c.ap = ap
    return c


@pytest.mark.parametrize("d", [16, 20])
@pytest.mark.parametrize("ld", [32, 64, 128, 256])
def test_row_widths(d, ld):
    _run_case(_case("d%d_ld%d" % (d, ld), d, ld, 5, seed=d + ld))


@pytest.mark.parametrize("attn,ap", [(3, 4), (5, 8), (16, 16), (17, 32), (3, 32), (5, 32), (16, 32)])
def test_attention_widths(attn, ap):
    _run_case(_case("attn%d_ap%d" % (attn, ap), 16, 32, attn, ap=ap, seed=attn + ap))


def test_tight_rows_ld_equals_d():
    _run_case(_case("d16_ld16", 16, 16, 5, seed=3))
    _run_case(_case("d64_ld64", 64, 64, 5, seed=4))


def _one_edge_case():
    c = _case("one_edge", 16, 32, 5, seed=5)
    hop = lr.static_hop(np.array([[1, 7, 2, 9, 3, 0]]), 4, 1)
    A = dict(dst_ptr=np.array([0, 1], np.int32), src_idx=np.array([3], np.int32), rel=np.array([2], np.int32),
             row_of_dst=np.array([1], np.int32))
    return c, hop, A


def test_one_destination_with_one_edge():
    c, hop, A = _one_edge_case()
    x = lr.inputs(c, 0, hop)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    agg, alpha = _call(c, A, X)
    _check("one edge", c, agg, lr.forward(hop, *(x[kk] for kk in KEYS)))
    assert alpha.shape == (1,) and 0.0 < float(alpha[0]) < 1.0


def test_hub_next_to_many_one_edge_destinations():
    """layer_ref's hub regime: destinations of 1, 127, 128, 129, 256, 257 and 3000 in-edges (3000: 24 chunks; 128: the longest that is
    not cut) among thousands of one-edge leaves.  A destination's row does not depend on what else the call carries: the hubs alone,
    and every third destination, give bit for bit the rows of the full call."""
    from red_gnn_amd import engine
    case = lr.CASES["hubs"]()
    hop, A, x, X, agg = _run_case(case)
    length = np.diff(A["dst_ptr"].astype(np.int64))
    n_hub, n_chunks, longest = engine.digraph_chunks(A["dst_ptr"])
    assert longest > 2 * engine.DIGRAPH_CHUNK and n_hub >= 4 and (length == 1).sum() > 1000 and (length == engine.DIGRAPH_CHUNK).any()
    for pick in (np.nonzero(length > engine.DIGRAPH_CHUNK)[0], np.arange(0, len(length), 3), np.array([int(length.argmax())])):
        at = np.concatenate([np.arange(A["dst_ptr"][o], A["dst_ptr"][o + 1]) for o in pick])
        ptr = np.zeros(len(pick) + 1, np.int32)
        ptr[1:] = np.cumsum(length[pick])
        sub = dict(dst_ptr=ptr, src_idx=A["src_idx"][at], rel=A["rel"][at], row_of_dst=A["row_of_dst"][pick])
        part, _ = _call(case, sub, X)
        assert torch.equal(part, agg[torch.as_tensor(pick).cuda()]), "a destination's row depends on the rest of the call"


def test_engine_wrapper_checks_and_matches():
    """engine.digraph_layer_fwd: the raw call's bits, zero rows for destinations without edges, E == 0, and ValueError for indices
    outside their tables."""
    from red_gnn_amd import engine
    case = _case("wrapper", 20, 32, 5, seed=6)
    old, new, edges, _ = lr.hops(case)[1]
    hop, A = _by_destination(edges, len(old), len(new))
    x = lr.inputs(case, 1, hop)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    raw, raw_alpha = _call(case, A, X)
    D = {k: _dev(v, torch.int32) for k, v in A.items()}
    tabs = (X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], case.attn_dim)
    agg, alpha = engine.digraph_layer_fwd(D["dst_ptr"], D["src_idx"], D["rel"], D["row_of_dst"], *tabs)
    assert torch.equal(agg, raw) and torch.equal(alpha, raw_alpha)
    # two destinations without edges appended: their rows are zero, the others keep their bits
    ptr2 = torch.cat([D["dst_ptr"], D["dst_ptr"][-1:].repeat(2)])
    rows2 = torch.cat([D["row_of_dst"], torch.zeros(2, dtype=torch.int32, device="cuda")])
    agg2, _ = engine.digraph_layer_fwd(ptr2, D["src_idx"], D["rel"], rows2, *tabs)
    assert torch.equal(agg2[:-2], raw) and not agg2[-2:].any()
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    agg0, alpha0 = engine.digraph_layer_fwd(torch.zeros(4, dtype=torch.int32, device="cuda"), none, none, rows2[:3], *tabs)
    assert agg0.shape == (3, case.ld) and not agg0.any() and alpha0.numel() == 0
    for name, bad in (("src_idx", X["hidden"].shape[0]), ("rel", X["rela"].shape[0]), ("row_of_dst", X["a_q"].shape[0]), ("src_idx", -1)):
        args = dict(D)
        args[name] = D[name].clone()
        args[name][0] = bad
        with pytest.raises(ValueError, match=name + " out of range"):
            engine.digraph_layer_fwd(args["dst_ptr"], args["src_idx"], args["rel"], args["row_of_dst"], *tabs)


def test_no_edges_launches_nothing():
    from red_gnn_amd import _lib
    c, hop, A = _one_edge_case()
    X = {kk: _dev(v) for kk, v in lr.inputs(c, 0, hop).items() if v is not None}
    empty = dict(dst_ptr=np.zeros(4, np.int32), src_idx=np.zeros(0, np.int32), rel=np.zeros(0, np.int32), row_of_dst=np.zeros(3, np.int32))
    agg, alpha = _call(c, empty, X)
    assert torch.isnan(agg).all() and alpha.numel() == 0          # success, and agg_out is left alone
    assert _lib.lib().rg_digraph_layer_fwd(*([0, 0] + [None] * 5 + [0, 0, 0, None, None, 16, 16, None, None, None, 4, None, None, 3] +
                                             [None] * 3 + [0, None])) == 0


def test_unsupported_attention_width_is_an_error_and_the_next_call_is_fine():
    from red_gnn_amd import _lib
    case = _case("ap20", 16, 32, 5, seed=7)
    old, new, edges, _ = lr.hops(case)[0]
    hop, A = _by_destination(edges, len(old), len(new))
    x = lr.inputs(case, 0, hop)
    good = {kk: _dev(v) for kk, v in x.items() if v is not None}
    case.attn_dim = case.ap = 20
    X = {kk: _dev(v) for kk, v in lr.inputs(case, 0, hop).items() if v is not None}
    with pytest.raises(_lib.NativeError, match="padded attention dim 20"):
        _call(case, A, X)
    case.attn_dim, case.ap = 5, 8
    agg, _ = _call(case, A, good)
    _check("after the error", case, agg, lr.forward(hop, *(x[kk] for kk in KEYS)))


def test_alpha_is_the_forwards_float_on_hop_1_of_a_real_digraph():
    """rd.alpha is what rg_explain_emit stored, the float rg_layer_fwd multiplied by; on the same inputs (hop 1: hidden = a_s = 0, the
    model's own tables) alpha_out has the same bits."""
    from red_gnn_amd import engine
    from red_gnn_amd.models import _pad4, pad_attn
    from tests.test_explain_gpu import _loader, _model, _synthetic
    loader = _loader(_synthetic())
    for d, a in ((20, 5), (32, 17)):
        model = _model(loader, 2, d, a, "relu")
        rng = np.random.default_rng(d)
        subs, rels = rng.integers(0, loader.n_ent, 12), rng.integers(0, 2 * loader.n_rel, 12)
        rd = model.explain(subs, rels)
        ld, ap = max(16, _pad4(d)), pad_attn(a)
        first = rd.edges[:, 1] == 1
        e = rd.edges[first].long()
        assert e.shape[0] > 12 and bool((e[:, 2] == rd.q_sub[e[:, 0]]).all())          # every hop-1 edge starts at s
        keys, counts = torch.unique_consecutive(e[:, 0] * loader.n_ent + e[:, 4], return_counts=True)
        ptr = torch.zeros(keys.numel() + 1, dtype=torch.int32, device="cuda")
        ptr[1:] = torch.cumsum(counts, 0)
        a_r, a_q, rela_p = model.inference_tables(rd.q_rel, ld, ap)[0]
        layer = model.gnn_layers[0]
        i32 = lambda t: t.to(torch.int32).contiguous()
        with torch.no_grad():
            _, alpha = engine.digraph_layer_fwd(ptr, i32(e[:, 0]), i32(e[:, 3]), i32(keys // loader.n_ent), torch.zeros((12, ld), device="cuda"),
                                                rela_p.contiguous(), d, torch.zeros((12, ap), device="cuda"), a_r.contiguous(), a_q.contiguous(),
                                                layer.w_alpha.weight.detach().reshape(-1).contiguous(), layer.w_alpha.bias.detach().contiguous(), a)
        assert torch.equal(alpha, rd.alpha[first]), (d, a)
