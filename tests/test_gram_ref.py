"""The rg_gram_tn reference (tests/gram_ref.py) checked on the CPU: its geometry helpers by hand against csrc/gram.hip's formulas, its
two summation orders against each other in fp64, its fp32 evaluation (the kernel's summation shape) against the bound the GPU test
uses - so the bound is known to be one a correct fp32 implementation meets before a GPU is involved - and the GPU test's comparison
against three deliberately wrong copies of the operation, so it is known to reject a subtly wrong kernel."""
import functools
import re

import numpy as np
import pytest

from tests import gram_ref as gr


def test_geometry_by_hand():
    assert [gr.rows_per_wave(r) for r in (0, 1, 1024, 98304, 98305, 196608, 196609, 196613)] == [96, 96, 96, 96, 192, 192, 288, 288]
    assert [gr.mb_instance(m) for m in (1, 16, 17, 48, 64, 65, 80, 96, 97, 128, 144, 145, 176, 192)] == [1, 1, 2, 3, 4, 6, 6, 6, 9, 9, 9, 12, 12, 12]
    assert [gr.unroll(m) for m in (8, 32, 48, 64, 80, 96, 112, 144, 192)] == [8, 8, 4, 4, 3, 3, 2, 2, 2]
    assert all(gr.rows_per_wave(r) % (4 * u) == 0 for r in (0, 98305, 10 ** 7) for u in (2, 3, 4, 8))
    assert gr.n_terms(33000) == (96 + 256 + 3, 96 + 256 + 3 + 4) and gr.n_terms(98305)[0] == 192 + 259
    # 3 rows, m = 2, n = 1 by hand: out = [1*4 + 2*5 + 3*6, -1*4 + 0*5 + 1*6], colsum = [6, 0], S = the same with absolute values
    g, x = np.array([[1, -1], [2, 0], [3, 1]], np.float32), np.array([[4], [5], [-6]], np.float32)
    for dtype, order in ((np.float64, "blas"), (np.float64, "kernel"), (np.float32, "kernel")):
        r = gr.gram(g, x, dtype, order=order)
        assert r.out.dtype == dtype and r.out.tolist() == [[-4.0], [-10.0]] and r.colsum.tolist() == [6.0, 0.0]
        assert r.S["out"].tolist() == [[32.0], [10.0]] and r.S["colsum"].tolist() == [6.0, 2.0] and r.n == dict(out=355, colsum=359)
    assert gr.exact(g, x)[0].tolist() == [[-4], [-10]] and gr.exact(g, x)[1].tolist() == [6, 0]
    z = gr.gram(g[:0], x[:0], np.float32)
    assert z.out.shape == (2, 1) and not z.out.any() and not z.colsum.any() and not z.S["out"].any()
    # 196613 rows of +-3 stay below 2^24: every fp32 partial sum of an "int" case is exact, whatever the order
    assert 9 * 196613 < 2 ** 24 and max(c.n_rows for c in gr.CASES.values() if c.kind == "int") == 196613


@pytest.mark.parametrize("name", ["n_32x16_r33000", "n_1x64_r98305", "g_65x17_r1000", "r_96x32_r97"])
def test_kernel_order_equals_blas_in_fp64(name):
    """The summation in the kernel's shape and numpy's product are the same function: in fp64 they differ by rounding alone."""
    x = gr.inputs(gr.CASES[name])
    a, b = gr.gram(x["g"], x["x"], order="kernel"), gr.gram(x["g"], x["x"], order="blas")
    for o in ("out", "colsum"):
        assert (np.abs(getattr(a, o) - getattr(b, o)) <= 1e-12 * a.S[o]).all(), o
        assert np.array_equal(a.S[o], b.S[o])


@functools.lru_cache(maxsize=None)
def _ratios(name):
    """(ratio of out, ratio of colsum) of the fp32 evaluation in the kernel's shape against fp64."""
    case = gr.CASES[name]
    x = gr.inputs(case)
    r64, r32 = gr.gram(x["g"], x["x"]), gr.gram(x["g"], x["x"], np.float32)
    assert r32.out.dtype == r32.colsum.dtype == np.float32
    if case.kind == "int":
        ex = gr.exact(x["g"], x["x"])
        assert np.array_equal(r64.out, ex[0]) and np.array_equal(r64.colsum, ex[1]) and gr.agrees(case, r32.out, r32.colsum, ex) == (True, True)
    return (gr.worst_ratio(r32.out, r64.out, r64.S["out"], r64.n["out"], gr.N0_GRAM),
            gr.worst_ratio(r32.colsum, r64.colsum, r64.S["colsum"], r64.n["colsum"], gr.N0_COLSUM))


# the fp32 evaluation walks the rows one by one: the "int" cases beyond 1000 rows (exact in any order, see test_geometry_by_hand)
# run it at the narrow shape only
_CHEAP = [c.name for c in gr.CASES.values() if c.kind == "normal" or c.n_rows <= 1000 or c.m == 8]
_GROUPS = sorted({gr.CASES[n].group for n in _CHEAP if gr.CASES[n].kind == "int"})


@pytest.mark.parametrize("which", [n for n in _CHEAP if gr.CASES[n].kind == "normal"] + _GROUPS)
def test_fp32_reference_within_its_bound(which):
    """The reference evaluated in np.float32 in the kernel's summation shape against its fp64 self: the ratio
    |ref32 - ref64| / ((n + n0) u S) stays below REF32_WORST_RATIO_GRAM for every element of both outputs of every case ("normal"
    cases one by one, the "int" cases by group: they measure 0 and equal the int64 product), i.e. the GPU's bound (4 x that) is one a
    correct fp32 implementation meets with a factor 4 to spare.  Prints the ratios."""
    names = [which] if which in gr.CASES else [n for n in _CHEAP if gr.CASES[n].group == which and gr.CASES[n].kind == "int"]
    for name in names:
        r = _ratios(name)
        if which in gr.CASES or max(r) > 0:
            print("%s: out=%.3g colsum=%.3g" % ((name,) + r))
        assert max(r) <= gr.REF32_WORST_RATIO_GRAM, (name, r)
        assert gr.CASES[name].kind == "normal" or r == (0.0, 0.0)
    if which not in gr.CASES:
        print("%s: %d exact cases, all ratios 0" % (which, len(names)))


def test_large_int_cases_are_exact_in_fp32():
    """The "int" cases the row-by-row evaluation skips: a plain fp32 product (any order) equals the int64 one."""
    for c in gr.CASES.values():
        if c.name not in _CHEAP:
            x = gr.inputs(c)
            ex = gr.exact(x["g"], x["x"])
            assert 9 * c.n_rows < 2 ** 24 and np.array_equal((x["g"].T @ x["x"]).astype(np.float64), ex[0])
            assert np.array_equal(x["g"].sum(0, dtype=np.float32).astype(np.float64), ex[1])


def test_recorded_ratio_is_the_measured_one():
    """REF32_WORST_RATIO_GRAM is the table's worst figure rounded up, not a looser guess: within 1.25 x of the worst normal case."""
    worst = max(max(_ratios(n)) for n in _CHEAP if gr.CASES[n].kind == "normal")
    assert worst <= gr.REF32_WORST_RATIO_GRAM <= 1.25 * worst, worst
    assert gr.C_BOUND_GRAM == 4.0 * gr.REF32_WORST_RATIO_GRAM


_FAULT_CASES = [
    # (fault, case, out fails, colsum fails)
    ("drop_tail_row", "g_16x16_r1000", True, True), ("drop_tail_row", "g_177x49_r1000", True, True),
    ("drop_tail_row", "r_8x64_r1", True, True), ("drop_tail_row", "r_8x64_r33", True, True), ("drop_tail_row", "r_96x32_r97", True, True),
    ("drop_tail_row", "r_8x64_r98305", True, True), ("drop_tail_row", "r_8x64_r196613", True, True),
    ("drop_tail_row", "n_32x16_r33000", True, True), ("drop_tail_row", "n_80x40_r33000", True, True),
    ("drop_tail_row", "n_32x16_r98305", True, True), ("drop_tail_row", "n_1x64_r33000", True, True),
    ("colsum_three_quarters", "g_1x1_r1000", False, True), ("colsum_three_quarters", "g_96x32_r1000", False, True),
    ("colsum_three_quarters", "r_48x16_r5", False, True), ("colsum_three_quarters", "n_32x16_r33000", False, True),
    ("colsum_three_quarters", "n_1x64_r98305", False, True),
    ("narrow_geometry", "g_65x16_r1000", True, True), ("narrow_geometry", "g_80x33_r1000", True, True),
    ("narrow_geometry", "g_97x64_r1000", True, True), ("narrow_geometry", "g_128x1_r1000", True, True),
    ("narrow_geometry", "g_145x48_r1000", True, True), ("narrow_geometry", "g_176x17_r1000", True, True),
    ("narrow_geometry", "n_80x40_r33000", True, True), ("narrow_geometry", "n_120x40_r33000", True, True),
    # where the instance is as wide as m needs the two geometries are one: nothing to catch
    ("narrow_geometry", "g_96x32_r1000", False, False), ("narrow_geometry", "g_64x64_r1000", False, False),
    ("narrow_geometry", "g_192x64_r1000", False, False),
]


@pytest.mark.parametrize("fault,name,out_fails,cs_fails", _FAULT_CASES)
def test_comparison_rejects_a_wrong_kernel(fault, name, out_fails, cs_fails):
    """The GPU test can fail: the fp32 evaluation with one thing wrong - the last row of the last non-empty wave skipped; the fourth
    quarter slot left out of the column sum; the partials read back with the geometry m needs instead of the instance's - put in the
    GPU result's place fails the comparison tests/test_gram_gpu.py applies (gram_ref.agrees: bitwise equality for "int" cases, the
    bound for "normal" ones) on each output the fault reaches, and the untouched output still passes."""
    case = gr.CASES[name]
    x = gr.inputs(case)
    ref = gr.exact(x["g"], x["x"]) if case.kind == "int" else gr.gram(x["g"], x["x"])
    good = gr.gram(x["g"], x["x"], np.float32)
    assert gr.agrees(case, good.out, good.colsum, ref) == (True, True)
    if fault == "drop_tail_row":
        assert x["g"][-1].any() and x["x"][-1].any()      # the dropped row carries something
    bad = gr.gram(x["g"], x["x"], np.float32, fault=fault)
    assert gr.agrees(case, bad.out, bad.colsum, ref) == (not out_fails, not cs_fails)


def test_bound_with_n_rows_would_pass_a_dropped_row():
    """Why n is the longest chain and not n_rows: with n = n_rows the bound admits a good part of the elements of a result that lacks
    one row of 33000 (every element whose dropped product is below a tenth of a typical one); with the chain length next to none."""
    case = gr.CASES["n_32x16_r33000"]
    x = gr.inputs(case)
    ref, bad = gr.gram(x["g"], x["x"]), gr.gram(x["g"], x["x"], np.float32, fault="drop_tail_row")
    err = np.abs(bad.out.astype(np.float64) - ref.out)
    tight = err <= gr.bound(ref.S["out"], ref.n["out"], gr.N0_GRAM, gr.C_BOUND_GRAM)
    loose = err <= gr.bound(ref.S["out"], case.n_rows, gr.N0_GRAM, gr.C_BOUND_GRAM)
    print("within the bound: n = chain %.3f, n = n_rows %.3f" % (tight.mean(), loose.mean()))
    assert tight.mean() < 0.01 and loose.mean() > 0.1


def test_cited_lines_say_what_the_tables_say():
    """The ``why`` columns cite lines of csrc/gram.hip, engine.py and models.py: the lines still hold what they are cited for."""
    import os
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "red-gnn_amd")
    lines = lambda rel: [""] + open(os.path.join(root, rel)).read().split("\n")
    hip, eng, mod = lines("csrc/gram.hip"), lines("engine.py"), lines("models.py")
    for no, text in ((18, "GRAM_WAVES ="), (36, "r_end ="), (47, "m_ok[a] ="), (49, "n_ok[b] ="), (51, "constexpr int U ="), (52, "r0 += 4 * U"),
                     (56, "r0 + 4 * u + kq"), (57, "ok = r < r_end"), (113, "w += 4"), (121, "red[192 + el]"), (137, "launch<MB, 1>"),
                     (138, "launch<MB, 2>"), (139, "launch<MB, 3>"), (140, "launch<MB, 4>"), (146, "mb_instance"), (164, "A.rows_per_wave ="),
                     (169, "case 1:"), (170, "case 2:"), (171, "case 3:"), (172, "case 4:"), (173, "case 5: case 6:"), (174, "case 7: case 8: case 9:"),
                     (175, "default: rc = launch_n<12>"), (181, "mb_used * 16")):
        assert text in hip[no], (no, hip[no])
    for no, text in ((743, "range(0, m, 192)"), (754, "colsum and n0 == 0"), (762, "cs[m0:m0 + mc] = cs_t")):
        assert text in eng[no], (no, eng[no])
    for no, text in ((66, "g.t() @ x"), (68, "engine.gram_tn(g, x)"), (90, "g @ weight"), (91, "_gram_tn(g, x)"), (92, "g.sum(0)"),
                     (164, "_gram_tn(g_as[:, :a], hidden)"), (165, "engine.rows_addmm"), (166, "n >= _TALL_ROWS and ctx.prev_idx is not None"),
                     (171, "ws.view(n, 5, d)[:, 3]"), (172, "engine.gram_tn(dgi, x, colsum=True)"), (173, "engine.gram_tn(dgi[:, :2 * d], h0"),
                     (174, "engine.gram_tn(dpre, agg)"), (175, "torch.cat([g_rz, g_n])"), (176, "n >= _FUSED_BWD_ROWS"), (180, "n >= _TALL_ROWS"),
                     (181, "engine.gram_tn(dgh, h0, colsum=True)"), (182, "engine.gram_tn(dpre, agg)"), (185, "dgi.sum(0), dgh.sum(0)"),
                     (187, "_thnn_fused_gru_cell_backward"), (201, "_gram_tn(dgi, x), _gram_tn(dgh, h0)"), (202, "_gram_tn(dpre, agg)"),
                     (519, "engine.prefer_blas(n_new)")):
        assert text in mod[no], (no, mod[no])


def test_table_covers_what_it_names():
    """Between them the ``why`` columns name every case of the switch (mb), every launch_n branch, each U, the rows_per_wave step and
    the call forms; the table holds the shapes the issue lists."""
    C = list(gr.CASES.values())
    assert all(c.why for c in C)
    grid = [c for c in C if c.group == "grid"]
    assert len(grid) == 192 and {c.n_rows for c in grid} == {1000} and {c.kind for c in grid} == {"int"}
    assert {(c.m + 15) // 16 for c in grid} == set(range(1, 13)) and {(c.n + 15) // 16 for c in grid} == {1, 2, 3, 4}
    assert {gr.mb_instance(c.m) for c in grid} == {1, 2, 3, 4, 6, 9, 12} and {c.m for c in grid} >= {1, 192} and {c.n for c in grid} >= {1, 64}
    why = " ".join(c.why for c in C)
    for mb in range(1, 13):
        assert "switch (mb) case %d " % mb in why
    assert {int(v) for v in re.findall(r"gram\.hip:(\d+) switch", why)} == {169, 170, 171, 172, 173, 174, 175}
    assert {int(v) for v in re.findall(r"gram\.hip:(\d+) launch_n", why)} == {137, 138, 139, 140}
    assert {int(v) for v in re.findall(r"MB = \d+, U = (\d)", why)} == {2, 3, 4, 8} and "rows_per_wave steps from 96 to 192" in why
    assert "remap" in why and "models.py:171-173" in why and "engine.py:743-762" in why
    rows = [c for c in C if c.group == "rows"]
    assert {(c.m, c.n) for c in rows} == set(gr.ROW_SHAPES) and {gr.unroll(c.m) for c in rows} == {2, 3, 4, 8}
    for m, n in gr.ROW_SHAPES:
        u = gr.unroll(m)
        assert {c.n_rows for c in rows if c.m == m} == {0, 1, 3, 4, 5, 4 * u - 1, 4 * u, 4 * u + 1, 95, 96, 97, 98303, 98304, 98305, 196613}
    # tails that are no multiple of 4 U for U = 3 (MB 6) and U = 8 (MB 2)
    assert any(gr.mb_instance(c.m) == 6 and (c.n_rows % gr.rows_per_wave(c.n_rows)) % 12 for c in C)
    assert any(gr.mb_instance(c.m) == 2 and (c.n_rows % gr.rows_per_wave(c.n_rows)) % 32 for c in C)
    assert {(c.m, c.n, c.d) for c in C if c.form == "step"} == {(32, 16, 16), (80, 40, 40), (128, 64, 64)}
    assert {(c.m, c.n) for c in C if c.form == "engine"} == {(193, 65), (200, 20), (30, 130), (256, 128), (384, 128)}
    normal = [c for c in C if c.kind == "normal"]
    assert {(c.m, c.n) for c in normal} == {(1, 64), (32, 16), (80, 40), (96, 32), (120, 40), (168, 56), (192, 64)}
    assert {c.n_rows for c in normal} == {33000, 98305} and len(normal) == 14
    x = gr.inputs(gr.CASES["n_192x64_r33000"])
    col = np.abs(x["g"]).mean(0)
    assert col.max() / col.min() > 1e3 and x["g"].dtype == x["x"].dtype == np.float32
    x = gr.inputs(gr.CASES["g_192x64_r1000"])
    assert set(np.unique(x["g"])) == set(np.unique(x["x"])) == set(np.arange(-3.0, 4.0))
