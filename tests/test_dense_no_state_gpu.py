"""rg_dense_fwd without hidden_out: on the last layer (W_final given, no Ws_next) the caller may pass hidden_out = NULL, and the six fused
dense kernels (d <= 64 and d = 128, precisions f32 / f16x2 / f16x3) then skip the new state's stores.  The scores must be bit for bit
what the call with hidden_out writes; hidden_out = NULL together with Ws_next is an argument error.
Rows: 1, 15, 16, 17 (around the 16-row tile) and 1000 (several workgroups), with and without prev_idx.  Wall time on an MI355X: ~1 s."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N_ENT = 64
PRECISIONS = {"f32": 0, "f16x2": 1, "f16x3": 2}


def _inputs(n, d, with_prev, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    ld = max(16, (d + 3) // 4 * 4)
    n_old = max(n // 2, 1)
    agg, hprev = torch.zeros(n, ld), torch.zeros(n_old, ld)
    agg[:, :d], hprev[:, :d] = r(n, d), torch.tanh(r(n_old, d))
    prev = torch.full((n,), -1, dtype=torch.int32)
    prev[::2][:n_old] = torch.arange(min(n_old, (n + 1) // 2), dtype=torch.int32)      # every other node carries an old state
    perm = torch.randperm(n * 7, generator=g)[:n].sort().values                          # distinct (query, entity) pairs, sorted
    nodes = torch.stack([perm // N_ENT, perm % N_ENT], 1).to(torch.int32)
    s = d ** -0.5
    X = dict(agg=agg, hprev=hprev, prev=prev if with_prev else None, W_h=r(d, d) * s, w_ih=r(3 * d, d) * s, w_hh=r(3 * d, d) * s,
             b_ih=r(3 * d) * 0.1, b_hh=r(3 * d) * 0.1, W_final=r(d) * s, Ws=r(5, d) * s, nodes=nodes)
    return ld, {k: None if v is None else v.cuda().contiguous() for k, v in X.items()}


def _call(n, d, ld, X, precision, hidden_out, with_ws=False):
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n_q = (n * 7 + N_ENT - 1) // N_ENT
    scores = torch.zeros(n_q * N_ENT, dtype=torch.float32, device="cuda")
    a_s = torch.zeros((n, 8), dtype=torch.float32, device="cuda") if with_ws else None
    nb = int(L.rg_dense_scratch_bytes(d, precision))
    scratch = torch.empty(max(nb, 1), dtype=torch.uint8, device="cuda") if nb else None
    _lib.check(L.rg_dense_fwd(n, d, ld, p(X["agg"]), p(X["hprev"] if X["prev"] is not None else None), p(X["prev"]), p(X["W_h"]), 1,
                              p(X["w_ih"]), p(X["w_hh"]), p(X["b_ih"]), p(X["b_hh"]), p(X["Ws"]) if with_ws else None, 5 if with_ws else 0,
                              8 if with_ws else 0, p(a_s), p(X["W_final"]), p(X["nodes"]), N_ENT, p(scores), p(hidden_out), precision,
                              p(scratch), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return scores


@pytest.mark.parametrize("with_prev", [False, True])
@pytest.mark.parametrize("d", [64, 48, 128])
@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_scores_bitwise_equal_without_hidden_out(precision, d, with_prev):
    for n in (1, 15, 16, 17, 1000):
        ld, X = _inputs(n, d, with_prev, seed=1000 * d + n)
        hidden = torch.full((n, ld), float("nan"), dtype=torch.float32, device="cuda")
        with_state = _call(n, d, ld, X, PRECISIONS[precision], hidden)
        without = _call(n, d, ld, X, PRECISIONS[precision], None)
        assert not torch.isnan(hidden[:, :d]).any() and with_state.abs().sum() > 0, (precision, d, n)
        assert torch.equal(with_state, without), "scores differ without hidden_out (%s, d=%d, n=%d)" % (precision, d, n)


@pytest.mark.parametrize("precision", list(PRECISIONS))
def test_no_hidden_out_with_next_layer_is_an_error(precision):
    from red_gnn_amd import _lib
    ld, X = _inputs(17, 64, True, seed=3)
    with pytest.raises(_lib.NativeError, match="hidden_out is NULL"):
        _call(17, 64, ld, X, PRECISIONS[precision], None, with_ws=True)


def test_engine_dense_fwd_want_hidden_false():
    """engine.dense_fwd(want_hidden=False) allocates no state and returns the same scores."""
    import types
    from red_gnn_amd import engine as eng
    n, d = 100, 64
    ld, X = _inputs(n, d, True, seed=9)
    gate = types.SimpleNamespace(weight_ih_l0=X["w_ih"], weight_hh_l0=X["w_hh"], bias_ih_l0=X["b_ih"], bias_hh_l0=X["b_hh"])
    out = []
    for want in (True, False):
        scores = torch.zeros(((n * 7 + N_ENT - 1) // N_ENT) * N_ENT, dtype=torch.float32, device="cuda")
        h, a = eng.dense_fwd(X["agg"], X["hprev"], X["prev"], d, X["W_h"], "relu", gate, W_final=X["W_final"], nodes=X["nodes"],
                             n_ent=N_ENT, scores_all=scores, precision="f16x3", want_hidden=want)
        assert (h is not None) == want and a is None
        out.append(scores)
    assert torch.equal(out[0], out[1])
