"""rg_gram_tn called on its own - every kernel instance, every remap, every row-count edge, the call forms of models._DenseStep and
engine.gram_tn's tiling - against tests/gram_ref.py, over the case table defined there (each case's ``why`` cites the line it flips).

G and X are column blocks of wider buffers whose surrounding columns are NaN, followed by 8 NaN rows: a read outside the promised
region shows up as NaN.  ``out``, ``colsum`` and the scratch are pre-filled with NaN and every element must be written.  Nothing is
exempt from any comparison.

    "int" cases     entries in {-3 .. 3}: every partial sum is an integer below 2^24, so the result must EQUAL the int64 product bit
                    for bit (no tolerance), a second run must be bitwise the same, and so must the product without ``colsum``
    "normal" cases  |gpu - ref64| <= C_BOUND_GRAM (n + n0) u S + 1e-30 for every element of out and colsum, with n = the longest chain
                    of additions (rows_per_wave + 256 + 3), not n_rows (gram_ref's docstring), and C_BOUND_GRAM = 4 x 0.0005 = 0.002:
                    4 x what the numpy fp32 evaluation in the kernel's summation shape costs
                    (tests/test_gram_ref.py::test_fp32_reference_within_its_bound keeps that figure honest on the CPU)

The kernel's own worst ratios are printed per case (run with -s) and summarised in KERNEL_RATIOS below, for information only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gram_ref as gr

pytestmark = pytest.mark.gpu

# the kernel's worst |gpu - ref64| / ((n + n0) u S) over the 14 "normal" cases, as measured on an MI355X (information only; the
# assertions use C_BOUND_GRAM)
KERNEL_RATIOS = {"out": 0.00049, "colsum": 0.00024}      # n_192x64_r33000, n_168x56_r33000
# wall time of this file on an MI355X: 7.5 s (28 tests)

NAN = float("nan")
PAD_ROWS = 8


def _nan(*shape):
    return torch.full(shape, NAN, dtype=torch.float32, device="cuda")


def _embed(a, left, right):
    """``a`` [rows, w] as the column block left .. left + w of a NaN buffer [rows + 8, left + w + right]: (buffer, pointer of the block,
    row stride)."""
    rows, w = a.shape
    buf = _nan(rows + PAD_ROWS, left + w + right)
    buf[:rows, left:left + w] = torch.as_tensor(a).cuda()
    return buf, buf.data_ptr() + 4 * left, buf.stride(0)


_SCRATCH = []


def _scratch():
    """One scratch buffer of the largest size, shared by the file."""
    from red_gnn_amd import _lib
    if not _SCRATCH:
        _SCRATCH.append(torch.empty(_lib.lib().rg_gram_tn_scratch_bytes(gr.M_MAX, gr.N_MAX), dtype=torch.uint8, device="cuda"))
    return _SCRATCH[0]


def _call(g_ptr, ldg, m, x_ptr, ldx, n, n_rows, colsum=True):
    """rg_gram_tn into NaN-filled out / colsum with a NaN-filled scratch of exactly the required size: (out, colsum or None)."""
    from red_gnn_amd import _lib
    L = _lib.lib()
    nbytes = L.rg_gram_tn_scratch_bytes(m, n)
    assert nbytes == gr.GRAM_WAVES * 16 * gr.mb_instance(m) * (16 * ((n + 15) // 16) + 16) * 4
    scratch = _scratch()
    scratch[:nbytes].fill_(0xFF)      # four 0xFF bytes are a NaN
    out, cs = _nan(m, n), _nan(m) if colsum else None
    _lib.check(L.rg_gram_tn(C.c_void_p(g_ptr), ldg, m, C.c_void_p(x_ptr), ldx, n, n_rows, _lib.ptr(out), _lib.ptr(cs), _lib.ptr(scratch), nbytes,
                            _lib.stream_ptr()))
    return out, cs


def _exact_case(case, x=None):
    """An "int" case through a direct call: equal to the int64 product, twice, with and without colsum."""
    x = gr.inputs(case) if x is None else x
    m, n, r = case.m, case.n, case.n_rows
    gbuf, gp, ldg = _embed(x["g"], 8, 16)
    xbuf, xp, ldx = _embed(x["x"], 4, 4)
    out, cs = _call(gp, ldg, m, xp, ldx, n, r)
    want_out, want_cs = (torch.as_tensor(t.astype(np.float32)).cuda() for t in gr.exact(x["g"], x["x"]))
    bad = lambda got, want: "%s: %d of %d elements differ (%d NaN); why: %s" % (case.name, int((got != want).sum()), want.numel(),
                                                                                 int(torch.isnan(got).sum()), case.why)
    assert torch.equal(out, want_out), "out " + bad(out, want_out)
    assert torch.equal(cs, want_cs), "colsum " + bad(cs, want_cs)
    out2, cs2 = _call(gp, ldg, m, xp, ldx, n, r)
    assert torch.equal(out2, out) and torch.equal(cs2, cs), case.name + ": second run differs"
    out3, _ = _call(gp, ldg, m, xp, ldx, n, r, colsum=False)
    assert torch.equal(out3, out), case.name + ": the product depends on the colsum option"
    if r == 0:
        assert not out.any() and not cs.any()
    return out, cs


def test_every_instance_and_remap_is_exact():
    """m in {16 k - 15, 16 k : k = 1 .. 12} x n in {16 k - 15, 16 k : k = 1 .. 4} at 1000 rows: every case of the switch (mb) - the
    instances MB = 1, 2, 3, 4, 6, 9, 12 and the remaps 5 -> 6, 7 / 8 -> 9, 10 / 11 -> 12, where the partials and the combine's mp take
    the wider instance's geometry -, every launch_n branch, m = 1 and n = 1."""
    cases = [c for c in gr.CASES.values() if c.group == "grid"]
    assert len(cases) == 192
    for case in cases:
        _exact_case(case)
    torch.cuda.synchronize()


@pytest.mark.parametrize("m,n", gr.ROW_SHAPES)
def test_row_counts_are_exact(m, n):
    """One shape per unroll depth U = 8, 4, 3, 2 at n_rows in {0, 1, 3, 4, 5, 4U - 1, 4U, 4U + 1, 95, 96, 97, 98303, 98304, 98305, 196613}:
    no rows (all-zero out and colsum), less than one MFMA K step, tails around one loop iteration, around wave 0's range, around the
    step of rows_per_wave from 96 to 192 (half the waves with an empty range) and a last wave whose tail is no multiple of 4 U."""
    cases = [c for c in gr.CASES.values() if c.group == "rows" and (c.m, c.n) == (m, n)]
    assert len(cases) == 15
    for case in cases:
        _exact_case(case)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d", gr.STEP_D)
def test_dense_step_call_forms_are_exact(d):
    """The views models._DenseStep.backward passes on its rg_dense_train_bwd2 route: G = dgi[:, :2d] with ldg = 3d, X =
    ws.view(n, 5, d)[:, 3] with ldx = 5d and a pointer offset of 3d floats; dgi's n block and the other four workspace blocks are NaN.
    Directly and through engine.gram_tn on the same views."""
    from red_gnn_amd import engine
    case = next(c for c in gr.CASES.values() if c.form == "step" and c.d == d)
    x = gr.inputs(case)
    r = case.n_rows
    dgi, ws = _nan(r + PAD_ROWS, 3 * d), _nan(r + PAD_ROWS, 5 * d)
    dgi[:r, :2 * d] = torch.as_tensor(x["g"]).cuda()
    ws[:r, 3 * d:4 * d] = torch.as_tensor(x["x"]).cuda()
    want_out, want_cs = (torch.as_tensor(t.astype(np.float32)).cuda() for t in gr.exact(x["g"], x["x"]))
    out, cs = _call(dgi.data_ptr(), 3 * d, 2 * d, ws.data_ptr() + 4 * 3 * d, 5 * d, d, r)
    assert torch.equal(out, want_out) and torch.equal(cs, want_cs), case.name
    dgi_v, ws_v = dgi[:r], ws[:r]
    h0 = ws_v.view(r, 5, d)[:, 3]
    assert h0.data_ptr() == ws.data_ptr() + 12 * d and h0.stride(0) == 5 * d
    e_out, e_cs = engine.gram_tn(dgi_v[:, :2 * d], h0, colsum=True)
    assert torch.equal(e_out, want_out) and torch.equal(e_cs, want_cs), case.name + ": engine.gram_tn"
    assert torch.equal(engine.gram_tn(dgi_v[:, :2 * d], h0), want_out)
    torch.cuda.synchronize()


@pytest.mark.parametrize("m,n", gr.ENGINE_SHAPES)
def test_engine_tiling_is_exact(m, n, monkeypatch):
    """engine.gram_tn beyond 192 x 64: one call per 192 x 64 tile, the tiles copied into out and cs at their offsets, the column sum
    taken on the n0 == 0 tiles only - and the whole equal to the int64 product."""
    from red_gnn_amd import _lib, engine
    case = next(c for c in gr.CASES.values() if c.form == "engine" and (c.m, c.n) == (m, n))
    x = gr.inputs(case)
    r = case.n_rows
    gbuf, gp, ldg = _embed(x["g"], 8, 16)
    xbuf, xp, ldx = _embed(x["x"], 4, 4)
    L = _lib.lib()
    native, calls = L.rg_gram_tn, []

    def spy(g_ptr, ldg_, mc, x_ptr, ldx_, nc, n_rows, out, colsum, *rest):
        calls.append((g_ptr.value, ldg_, mc, x_ptr.value, ldx_, nc, n_rows, colsum is not None))
        return native(g_ptr, ldg_, mc, x_ptr, ldx_, nc, n_rows, out, colsum, *rest)
    monkeypatch.setattr(L, "rg_gram_tn", spy, raising=False)
    out, cs = engine.gram_tn(gbuf[:r, 8:8 + m], xbuf[:r, 4:4 + n], colsum=True)
    want = [(gp + 4 * m0, ldg, min(192, m - m0), xp + 4 * n0, ldx, min(64, n - n0), r, n0 == 0) for m0 in range(0, m, 192) for n0 in range(0, n, 64)]
    assert calls == want
    want_out, want_cs = (torch.as_tensor(t.astype(np.float32)).cuda() for t in gr.exact(x["g"], x["x"]))
    assert out.shape == (m, n) and cs.shape == (m,)
    assert torch.equal(out, want_out), "%s: out, %d elements differ" % (case.name, int((out != want_out).sum()))
    assert torch.equal(cs, want_cs), "%s: cs, %d elements differ" % (case.name, int((cs != want_cs).sum()))
    out2 = engine.gram_tn(gbuf[:r, 8:8 + m], xbuf[:r, 4:4 + n])
    assert torch.equal(out2, out) and len(calls) == 2 * len(want) and not any(c[-1] for c in calls[len(want):])
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", [c.name for c in gr.CASES.values() if c.kind == "normal"])
def test_rounding_within_the_bound(name):
    """Standard normal entries with per-column scales over 1e-3 .. 30 at 33000 and 98305 rows: every element of out and colsum within
    bound(S, n, n0, C_BOUND_GRAM) of fp64; bitwise reproducible."""
    case = gr.CASES[name]
    x = gr.inputs(case)
    m, n, r = case.m, case.n, case.n_rows
    gbuf, gp, ldg = _embed(x["g"], 8, 16)
    xbuf, xp, ldx = _embed(x["x"], 4, 4)
    out, cs = _call(gp, ldg, m, xp, ldx, n, r)
    ref = gr.gram(x["g"], x["x"])
    ratios = {}
    for o, got, n0 in (("out", out, gr.N0_GRAM), ("colsum", cs, gr.N0_COLSUM)):
        got = got.cpu().numpy().astype(np.float64)
        assert not np.isnan(got).any(), "%s %s: %d elements NaN (never written, or a read outside the promised region)" % (name, o, int(np.isnan(got).sum()))
        ratios[o] = gr.worst_ratio(got, getattr(ref, o), ref.S[o], ref.n[o], n0)
    print("%s: out=%.3g colsum=%.3g (allowed %.3g)" % (name, ratios["out"], ratios["colsum"], gr.C_BOUND_GRAM))
    ok_out, ok_cs = gr.agrees(case, out.cpu().numpy(), cs.cpu().numpy(), ref)
    assert ok_out and ok_cs, "%s: worst ratio out %.3g colsum %.3g, allowed %.3g; why: %s" % (name, ratios["out"], ratios["colsum"], gr.C_BOUND_GRAM, case.why)
    out2, cs2 = _call(gp, ldg, m, xp, ldx, n, r)
    assert torch.equal(out2, out) and torch.equal(cs2, cs), name + ": second run differs"
    assert torch.equal(_call(gp, ldg, m, xp, ldx, n, r, colsum=False)[0], out), name + ": the product depends on the colsum option"
    torch.cuda.synchronize()


def test_argument_errors_are_reported():
    """Unsupported arguments return non-zero with their message and launch nothing (out and colsum keep their NaN fill); an exact case
    run afterwards still matches."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    buf = torch.zeros(64 * 256, dtype=torch.float32, device="cuda")
    out, cs = _nan(192 * 64), _nan(192)
    scratch = _scratch()
    b, s, full = p(buf), _lib.stream_ptr(), scratch.numel()

    def call(ldg, m, ldx, n, out_t=out, nbytes=full):
        return L.rg_gram_tn(b, ldg, m, b, ldx, n, 16, p(out_t), p(cs), p(scratch), nbytes, s)
    for m in (0, 193):
        with pytest.raises(_lib.NativeError, match=r"rg_gram_tn: m=%d \(<= 192\) n=64 \(<= 64\): tile wider products over column blocks" % m):
            _lib.check(call(256, m, 64, 64))
    with pytest.raises(_lib.NativeError, match=r"rg_gram_tn: m=192 \(<= 192\) n=65 \(<= 64\)"):
        _lib.check(call(256, 192, 128, 65))
    with pytest.raises(_lib.NativeError, match=r"rg_gram_tn: ldg=47 ldx=64"):
        _lib.check(call(47, 48, 64, 16))
    need = L.rg_gram_tn_scratch_bytes(48, 16)
    with pytest.raises(_lib.NativeError, match=r"rg_gram_tn: scratch %d B < required %d B" % (need - 1, need)):
        _lib.check(call(48, 48, 16, 16, nbytes=need - 1))
    with pytest.raises(_lib.NativeError, match=r"rg_gram_tn: NULL argument"):
        _lib.check(call(48, 48, 16, 16, out_t=None))
    assert L.rg_gram_tn_scratch_bytes(0, 64) == L.rg_gram_tn_scratch_bytes(193, 64) == L.rg_gram_tn_scratch_bytes(192, 65) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(cs).all() and not buf.any()
    _exact_case(gr.CASES["g_81x33_r1000"])
    torch.cuda.synchronize()
