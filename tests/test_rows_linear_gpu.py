"""rg_rows_linear on the MI355X (-m gpu): x W^T (+ bias) against float64, and the property it exists for: a row's result does not
depend on the number of rows of the call.

Tolerance: every output is one fp32 fmaf chain of k terms, so |out - ref| <= k * 2^-23 * sum_j |x_j w_j| (the standard bound
gamma_k of a recursive sum, with the final bias add), plus 2^-149 for a subnormal result."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref_and_bound(x, w, b):
    x64, w64 = x.double().cpu().numpy(), w.double().cpu().numpy()
    ref = x64 @ w64.T + (0.0 if b is None else b.double().cpu().numpy())
    mag = np.abs(x64) @ np.abs(w64).T + (0.0 if b is None else np.abs(b.double().cpu().numpy()))
    return ref, (x.shape[1] + 1) * 2.0 ** -23 * mag + 2.0 ** -149


# (k, n, bias): float4 and scalar row loads, one column, columns that are no multiple of 4, column tiles (k * n * 4 B above 64 KB)
@pytest.mark.parametrize("k,n,bias", [(32, 8, False), (64, 64, False), (32, 1, True), (96, 20, True), (30, 5, True), (1, 3, False),
                                      (1100, 40, True), (129, 130, False)])
def test_against_float64_and_across_row_counts(k, n, bias):
    from red_gnn_amd import engine
    g = torch.Generator().manual_seed(k * 131 + n)
    N = 3001
    x = torch.randn(N, k, generator=g).cuda()
    w = torch.randn(n, k, generator=g).cuda()
    b = torch.randn(n, generator=g).cuda() if bias else None
    out = engine.rows_linear(x, w, b)
    assert out.shape == (N, n) and out.dtype == torch.float32
    ref, bound = _ref_and_bound(x, w, b)
    err = np.abs(out.double().cpu().numpy() - ref)
    print("k=%d n=%d: largest error / bound %.3g" % (k, n, float((err / bound).max())))
    assert (err <= bound).all()
    for m in (1, 2, 3, 5, 16, 33, 64, 300, 1000):
        assert torch.equal(engine.rows_linear(x[:m].contiguous(), w, b), out[:m]), m
        assert torch.equal(engine.rows_linear(x[1000:1000 + m], w, b), out[1000:1000 + m]), m       # (a view: another base address)


def test_spaced_rows_transposed_weights_and_no_rows():
    from red_gnn_amd import engine
    g = torch.Generator().manual_seed(5)
    wide = torch.randn(500, 24, generator=g).cuda()
    w = torch.randn(20, 7, generator=g).cuda().t()                       # [7, 20], not contiguous
    out = engine.rows_linear(wide[:, :20], w)                            # row stride 24
    assert torch.equal(out, engine.rows_linear(wide[:, :20].contiguous(), w.contiguous()))
    odd = engine.rows_linear(wide[:, 1:21], w)                           # rows off 16-B alignment: the scalar loads, the same chain
    assert torch.equal(odd, engine.rows_linear(wide[:, 1:21].contiguous(), w))
    assert engine.rows_linear(wide[:0, :20], w).shape == (0, 7)
