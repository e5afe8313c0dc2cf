"""The message-passing kernels called on their own - rg_layer_fwd / rg_layer_bwd, rg_tlayer_*, rg_xlayer_* - against the fp64 per-edge
reference of tests/layer_ref.py, over the case table defined there (one case per host-side dispatch condition; each case's comment in
layer_ref.CASES cites the condition it flips).  Per hop: the frontier's node list must equal the CPU oracle's bit for bit, then every
element of every output (pad columns included, nothing exempt) must satisfy

    |gpu - ref64| <= C_BOUND * (n + n0) * u * S + 1e-30                (layer_ref's docstring defines S, n, n0)

C_BOUND = 4 x REF32_WORST_RATIO = 4 x 0.4 = 1.6: the plain-numpy fp32 evaluation of the reference costs at most 0.391 of (n + n0) u S
on these cases (an agg element; tests/test_layer_ref.py::test_fp32_reference_within_its_bound keeps that figure honest on the CPU).
The kernels' own worst ratios are printed per case (run with -s) and summarised in KERNEL_RATIOS below, for information only.
"""

import numpy as np
import pytest
import torch

from tests import layer_ref as lr

pytestmark = pytest.mark.gpu

# the kernels' worst |gpu - ref64| / ((n + n0) u S) per output over the whole table, as measured on an MI355X (information only; the
# assertion uses C_BOUND)
KERNEL_RATIOS = {"agg": 0.391, "grad_hidden": 0.193, "grad_rela": 0.23, "grad_time": 0.173, "grad_a_s": 0.0078, "grad_a_r": 0.0091,
                 "grad_a_q": 0.0078, "grad_w_alpha": 3.1e-4, "grad_b_alpha": 3.2e-4}
# wall time of this file on an MI355X: 5.4 s (41 tests)

KEYS = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")


def _dev(x, dtype=torch.float32):
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _setup(case):
    """(graph, frontier at level 0) of a case: engine.Graph / TemporalGraph, Frontier.reset / reset_nodes / set_window."""
    from red_gnn_amd import engine as eng
    if case.kind == "static":
        g = eng.Graph(case.n_ent, case.n_rel, case.triples)
    else:
        g = eng.TemporalGraph(case.n_ent, case.n_rela_rows, case.n_time, case.quads)
    fr = eng.Frontier(case.n_ent, case.B, n_levels=case.hops + 1)
    if case.kind == "windowed":
        fr.set_window(_dev(case.win_lo, torch.int32), _dev(case.win_hi, torch.int32), case.n_data)
    if case.reset == "subjects":
        fr.reset(_dev(case.nodes0[:, 1], torch.int32))
    else:
        fr.reset_nodes(_dev(case.nodes0, torch.int32))
    return g, fr


def _extra(case):
    """Device copies of the temporal / windowed per-query arrays."""
    if case.kind == "static":
        return {}
    e = dict(q_time=_dev(case.q_time, torch.int32))
    if case.kind == "windowed":
        e.update(loop_time=_dev(case.loop_time, torch.int32), row_time=_dev(case.row_time, torch.int32))
    return e


def _forward(case, g, fr, X, ex, n_new, walk):
    """The layer forward into an agg buffer pre-filled with NaN (every row must be written); static: through engine.layer_fwd_into."""
    from red_gnn_amd import _lib, engine as eng
    L, p = _lib.lib(), _lib.ptr
    agg = torch.full((n_new, case.ld), float("nan"), dtype=torch.float32, device="cuda")
    scratch = torch.empty(L.rg_layer_fwd_scratch_bytes(fr.handle, g.handle, case.ld), dtype=torch.uint8, device="cuda")
    common = (p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), case.ap, p(X["w_alpha"]), p(X["b_alpha"]), case.attn_dim, p(agg), p(scratch),
              scratch.numel())
    if case.kind == "static":
        eng.layer_fwd_into(fr, g, fr.level, n_new, X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"],
                           case.attn_dim, agg, scratch, walk=walk)
    elif case.kind == "temporal":
        _lib.check(L.rg_tlayer_fwd(fr.handle, g.handle, fr.level, n_new, p(ex["q_time"]), p(X["hidden"]), p(X["rela"]), p(X["time_tab"]),
                                   case.d, case.ld, *common, _lib.stream_ptr()))
    else:
        _lib.check(L.rg_xlayer_fwd(fr.handle, g.handle, fr.level, n_new, p(ex["q_time"]), p(ex["loop_time"]), p(ex["row_time"]), case.n_data,
                                   p(X["hidden"]), p(X["rela"]), p(X["time_tab"]), case.n_tab, case.d, case.ld, *common, _lib.stream_ptr()))
    return agg


def _backward(case, g, fr, X, ex, n_old, base, with_aq=True):
    """The layer backward with caller-made outputs: WRITTEN ones (grad_hidden, grad_a_s, grad_a_q) pre-filled with NaN, ACCUMULATED
    ones (the tables, grad_w_alpha, grad_b_alpha) pre-filled with ``base``."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    nan = lambda t: torch.full_like(t, float("nan"))
    out = dict(grad_hidden=nan(X["hidden"]), grad_a_s=nan(X["a_s"]), grad_a_q=nan(X["a_q"]) if with_aq else None,
               grad_rela=base["grad_rela"].clone(), grad_a_r=base["grad_a_r"].clone(), grad_w_alpha=base["grad_w_alpha"].clone(),
               grad_b_alpha=base["grad_b_alpha"].clone(), grad_time=None if case.kind == "static" else base["grad_time"].clone())
    head = (fr.handle, g.handle, fr.level, n_old)
    attn = (p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), case.ap, p(X["w_alpha"]), p(X["b_alpha"]), case.attn_dim, p(X["grad_agg"]))
    if case.kind == "static":
        nb = L.rg_layer_bwd_scratch_bytes(fr.handle, g.handle, case.ld, case.ap)
        scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
        _lib.check(L.rg_layer_bwd(*head, p(X["hidden"]), p(X["rela"]), case.d, case.ld, *attn, p(out["grad_hidden"]), p(out["grad_rela"]),
                                  p(out["grad_a_s"]), p(out["grad_a_r"]), p(out["grad_a_q"]), p(out["grad_w_alpha"]), p(out["grad_b_alpha"]),
                                  p(scratch), nb, _lib.stream_ptr()))
    else:
        nb = L.rg_tlayer_bwd_scratch_bytes(fr.handle, g.handle, case.ld, case.ap)
        scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
        tail = (p(out["grad_hidden"]), p(out["grad_rela"]), p(out["grad_time"]), p(out["grad_a_s"]), p(out["grad_a_r"]), p(out["grad_a_q"]),
                p(out["grad_w_alpha"]), p(scratch), nb, _lib.stream_ptr())
        if case.kind == "temporal":
            _lib.check(L.rg_tlayer_bwd(*head, p(ex["q_time"]), p(X["hidden"]), p(X["rela"]), p(X["time_tab"]), case.d, case.ld, *attn, *tail))
        else:
            _lib.check(L.rg_xlayer_bwd(*head, p(ex["q_time"]), p(ex["loop_time"]), p(ex["row_time"]), case.n_data, p(X["hidden"]), p(X["rela"]),
                                       p(X["time_tab"]), case.n_tab, case.d, case.ld, *attn, *tail))
    torch.cuda.synchronize()
    return out


def _check(what, gpu, ref, S, n, n0, base=None):
    """Every element of ``gpu`` within the bound of ``ref`` (+ ``base`` for an accumulated output: the base is one more term of the sum,
    |base| joins S; an element no edge reaches, S = 0, must still hold its base bit for bit).  Returns the worst ratio."""
    gpu = gpu.detach().cpu().numpy().astype(np.float64).reshape(np.shape(ref))
    assert not np.isnan(gpu).any(), "%s: %d elements were never written" % (what, int(np.isnan(gpu).sum()))
    ref, S = np.asarray(ref, np.float64), np.asarray(S, np.float64)
    n = np.broadcast_to(np.asarray(n, np.float64), ref.shape)
    if base is not None:
        b = base.detach().cpu().numpy().astype(np.float64).reshape(ref.shape)
        untouched = S == 0
        assert np.array_equal(gpu[untouched], b[untouched]), "%s: an element without edges lost its base" % what
        ref, S, n = ref + b, np.where(untouched, 0.0, S + np.abs(b)), n + 1
        gpu = np.where(untouched, ref, gpu)
    err = np.abs(gpu - ref)
    ok = err <= lr.bound(S, n, n0, lr.C_BOUND)
    ratio = lr.worst_ratio(gpu, ref, S, n, n0)
    assert ok.all(), ("%s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g); first at %s: gpu %.9g ref %.9g S %.3g n %d"
                      % (what, int((~ok).sum()), ok.size, ratio, lr.C_BOUND, np.argwhere(~ok)[0], gpu[~ok][0], ref[~ok][0], S[~ok][0],
                         int(n[~ok][0])))
    return ratio


@pytest.mark.parametrize("name", list(lr.CASES))
def test_layer_kernels_vs_reference(name):
    from red_gnn_amd import _lib, engine as eng
    case = lr.CASES[name]()
    g, fr = _setup(case)
    ex = _extra(case)
    rng = np.random.default_rng(99)
    for k, (old, new, edges, hop) in enumerate(lr.hops(case)):
        tag = "%s hop %d" % (name, k + 1)
        n_new, n_e, n_old = fr.expand(g)
        nodes, _, _ = fr.nodes()
        assert (n_old, n_e) == (hop.n_old, hop.E), tag
        assert np.array_equal(nodes.cpu().numpy().astype(np.int64), new), tag + ": frontier nodes differ from the oracle's"
        x = lr.inputs(case, k, hop)
        X = {kk: _dev(v) for kk, v in x.items()}
        ref_args = [hop] + [x[kk] for kk in KEYS]
        ratios = {}

        # ---- forward: every walk the library accepts gives bitwise the same agg; the plan is one of them
        f64 = lr.forward(*ref_args)
        walks = {}
        if case.kind == "static":
            for w in range(1, 8):
                try:
                    walks[w] = _forward(case, g, fr, X, ex, n_new, w)
                except _lib.NativeError:
                    pass
            plan = eng.layer_fwd_plan(fr, g, fr.level, n_old, n_new, n_e, case.ld)
            assert 1 in walks and plan in walks, (tag, plan, sorted(walks))
            has_packs = case.n_ent <= (1 << 20) and case.n_rela_rows < (1 << 12)      # graph.hip: word-parallel packs
            assert sorted(walks) == (list(range(1, 8)) if has_packs else [1]), (tag, sorted(walks))
            if name == "short_rows_dense":
                assert plan >= 2, plan      # layer_fwd.hip plan_walk: short rows take the word-parallel walk even when saturated
            auto = eng.layer_fwd(fr, g, fr.level, nodes, X["hidden"], X["rela"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"],
                                 X["b_alpha"], case.attn_dim)
            for w, a in walks.items():
                assert torch.equal(a, auto), "%s: walk %d differs bitwise from the library's pick (%d)" % (tag, w, plan)
        else:
            walks[1] = _forward(case, g, fr, X, ex, n_new, 1)
        ratios["agg"] = _check(tag + " agg", walks[1], f64.agg, f64.S["agg"], f64.n["agg"], lr.n0_of("agg", case.d, case.attn_dim))
        assert not walks[1][:, case.d:].any(), tag + ": pad columns of agg"

        # ---- backward
        b64 = lr.backward(*ref_args, x["grad_agg"])
        shapes = dict(grad_rela=X["rela"], grad_a_r=X["a_r"], grad_w_alpha=X["w_alpha"], grad_b_alpha=X["b_alpha"], grad_time=X["time_tab"])
        base = {o: None if t is None else _dev(rng.standard_normal(tuple(t.shape)) + 0.25) for o, t in shapes.items()}
        out = _backward(case, g, fr, X, ex, n_old, base)
        for o in lr.BWD_OUTPUTS:
            if getattr(b64, o) is None or (o == "grad_b_alpha" and case.kind != "static"):
                continue
            ratios[o] = _check("%s %s" % (tag, o), out[o], getattr(b64, o), b64.S[o], b64.n[o], lr.n0_of(o, case.d, case.attn_dim),
                               base=base.get(o))
        assert not out["grad_a_s"][:, case.attn_dim:].any() and not out["grad_a_q"][:, case.attn_dim:].any(), tag + ": pad columns"
        # deterministic outputs (registers -> one store) are bitwise equal across runs; grad_a_q = NULL is accepted
        again = _backward(case, g, fr, X, ex, n_old, base, with_aq=False)
        assert torch.equal(again["grad_hidden"], out["grad_hidden"]) and torch.equal(again["grad_a_s"], out["grad_a_s"]), tag
        print("%s (n_old %d, n_new %d, E %d): %s" % (tag, n_old, n_new, n_e, " ".join("%s=%.3g" % kv for kv in ratios.items())))
    fr.close()
    g.close()


@pytest.mark.parametrize("ap", [20, 24, 28])
def test_unsupported_attention_widths_are_errors(ap):
    """common.h with_ap4 has no case for ap / 4 in {5, 6, 7}: every layer entry point returns non-zero with a message, launches nothing,
    and the process stays usable (a supported call afterwards still matches the reference)."""
    from red_gnn_amd import _lib
    for name in ("b31_e97", "temporal"):
        case = lr.CASES[name]()
        g, fr = _setup(case)
        ex = _extra(case)
        old, new, edges, hop = lr.hops(case)[0]
        n_new, n_e, n_old = fr.expand(g)
        good = {kk: _dev(v) for kk, v in lr.inputs(case, 0, hop).items()}
        case.attn_dim = case.ap = ap
        X = {kk: _dev(v) for kk, v in lr.inputs(case, 0, hop).items()}
        base = {o: torch.zeros_like(t) for o, t in dict(grad_rela=X["rela"], grad_a_r=X["a_r"], grad_w_alpha=X["w_alpha"],
                                                        grad_b_alpha=X["b_alpha"], grad_time=X["time_tab"]).items() if t is not None}
        for call in (lambda: _forward(case, g, fr, X, ex, n_new, 1), lambda: _backward(case, g, fr, X, ex, n_old, base)):
            with pytest.raises(_lib.NativeError, match="padded attention dim %d" % ap):
                call()
        if case.kind == "static":
            with pytest.raises(_lib.NativeError, match="padded attention dim %d" % ap):
                _forward(case, g, fr, X, ex, n_new, 2)
        case.attn_dim, case.ap = 5, 8
        f64 = lr.forward(hop, *(lr.inputs(case, 0, hop)[kk] for kk in KEYS))
        _check(name + " agg after the errors", _forward(case, g, fr, good, ex, n_new, 1), f64.agg, f64.S["agg"], f64.n["agg"],
               lr.n0_of("agg", case.d, 5))
        fr.close()
        g.close()
