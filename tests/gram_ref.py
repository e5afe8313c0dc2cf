"""Plain-numpy reference of rg_gram_tn (what include/redgnn.h promises: out = G[:, :m]^T X[:, :n], colsum = G[:, :m].sum(0), the
weight and bias gradients of the dense training step), plus the case table the gram tests share.  TEST INFRASTRUCTURE.

``gram(g, x, dtype)`` follows tests/dense_ref.py: np.float64 is the reference, np.float32 - the same code in the same order - is the
yardstick of what a correct fp32 evaluation costs.  The fp32 evaluation sums in the kernel's shape, read from csrc/gram.hip:

    rows_per_wave = ceil(ceil(max(n_rows, 1) / 1024) / 96) * 96         (gram.hip:164; 1024 = GRAM_WAVES)
    wave w owns rows [w rows_per_wave, (w + 1) rows_per_wave) and adds its products in row order            (gram.hip:35-74)
    out = ((c0 + c1) + c2) + c3 with chain c = the partials of waves c, c + 4, c + 8, ... added in that order  (gram.hip:113, :121)
    colsum: per wave four quarter sums (rows j = kq mod 4 of the wave's range), joined (q0 + q1) + (q2 + q3), then the same four
    chains over the waves                                                                                    (gram.hip:69, :87, :115)

(order="blas" replaces the summation by numpy's matrix product: the fp64 default, since at 2^-53 the order does not show;
test_gram_ref.py holds the two fp64 orders against each other.)  Besides ``out`` [m, n] and ``colsum`` [m] the function returns, in
fp64, ``S`` = the same expression with every term replaced by its absolute value (|G|^T |X|, |G|.sum(0)) and ``n`` = the number of
terms summed along the LONGEST CHAIN of additions into an element:

    n(out)    = rows_per_wave + 256 + 3        a wave's rows, a chain's 256 partials, the three joins
    n(colsum) = n(out) + 4                     the four quarter slots add to it

NOT n_rows: the error of a sum grows with the length of its chains, not with the number of its terms, and with n = n_rows = 33000
the bound would be 90 x as wide - one dropped row of 33000 would pass it.  The bound is dense_ref's,

    |fp32 - fp64| <= c * (n + n0) * u * S + tiny          u = 2^-24, tiny = 1e-30 (S = 0: the value must be exactly 0)

with n0 = ``N0_GRAM`` = 1 (the rounding of the product itself) for out and ``N0_COLSUM`` = 0 for colsum.

Two kinds of inputs: "int" - entries uniform in {-3 .. 3} held as fp32: every product and every partial sum is an integer below
2^24 (9 x 196613 < 2^24), so ANY order of fp32 additions is exact and the kernel must equal ``exact`` (the int64 product) bit for
bit; "normal" - standard normal entries with a per-column scale spread over 1e-3 .. 30, held to the bound.
"""
import types

import numpy as np

from tests.dense_ref import TINY, U, bound, worst_ratio  # noqa: F401  (re-exported: the gram tests use this module alone)

GRAM_WAVES = 1024            # gram.hip:18 GRAM_BLOCKS * GRAM_T / 64
M_MAX, N_MAX = 192, 64       # one call; engine.gram_tn tiles wider products
N0_GRAM = 1
N0_COLSUM = 0
# measured: max over the whole case table, both outputs and all elements of |ref32 - ref64| / ((n + n0) u S), rounded up
# (test_gram_ref.py::test_fp32_reference_within_its_bound prints the per-case figures; the worst is an out entry of n_120x40_r33000,
# 0.00046; the worst colsum entry, n_168x56_r33000's, 0.00024; the "int" cases measure 0: they are exact).  So far below 1 because S
# adds absolute values where the rounding errors of a chain of ~355 additions mostly cancel.
REF32_WORST_RATIO_GRAM = 0.0005
# the GPU's allowance: 4 x the fp32 reference's own cost (the order of the four rows inside an MFMA K step is the hardware's), the
# factor dense_ref.C_BOUND and layer_ref.C_BOUND grant the GPU over the CPU fp32 path
C_BOUND_GRAM = 4.0 * REF32_WORST_RATIO_GRAM

FAULTS = ("drop_tail_row", "colsum_three_quarters", "narrow_geometry")


def rows_per_wave(n_rows):
    return -(-(-(-max(int(n_rows), 1) // GRAM_WAVES)) // 96) * 96


def mb_instance(m):
    """The MB the kernel is instantiated for (gram.hip:146, :168-176): 1, 2, 3, 4, 6, 9, 12."""
    mb = (m + 15) // 16
    return mb if mb <= 4 else 6 if mb <= 6 else 9 if mb <= 9 else 12


def unroll(m):
    """K steps per loop iteration (gram.hip:51)."""
    MB = mb_instance(m)
    return 2 if MB >= 9 else 3 if MB >= 6 else 4 if MB >= 3 else 8


def n_terms(n_rows):
    """(n of out, n of colsum): the longest chain of additions."""
    n = rows_per_wave(n_rows) + GRAM_WAVES // 4 + 3
    return n, n + 4


def exact(g, x):
    """(out, colsum) of integer-valued inputs as int64.  The product runs through the fp64 matrix product (integers below 2^53: exact in
    any order; numpy's int64 product is a hundred times slower)."""
    gd, xd = np.asarray(g, np.float64), np.asarray(x, np.float64)
    assert np.array_equal(gd, np.rint(gd)) and np.array_equal(xd, np.rint(xd))
    assert len(gd) * max(np.abs(gd).max(initial=0), 1) * max(np.abs(xd).max(initial=0), 1) < 2 ** 53
    return (gd.T @ xd).astype(np.int64), gd.astype(np.int64).sum(0)


def _chains(part, dt):
    """((c0 + c1) + c2) + c3 over part [W, ...]: chain c adds part[c], part[c + 4], ... in order (waves without rows hold zeros, which
    change no sum: they are left out)."""
    W = part.shape[0]
    pad = np.zeros((-(-W // 4) * 4,) + part.shape[1:], dt)
    pad[:W] = part
    pad = pad.reshape((-1, 4) + part.shape[1:])
    c = np.zeros((4,) + part.shape[1:], dt)
    for k in range(pad.shape[0]):
        c += pad[k]
    return ((c[0] + c[1]) + c[2]) + c[3]


def _kernel_order(dt, g, x, fault):
    n_rows, m = g.shape
    n = x.shape[1]
    if n_rows == 0:
        return np.zeros((m, n), dt), np.zeros(m, dt)
    rpw = rows_per_wave(n_rows)
    W = -(-n_rows // rpw)      # waves with rows; the others' partials are zero
    G, X = np.zeros((W * rpw, m), dt), np.zeros((W * rpw, n), dt)
    G[:n_rows], X[:n_rows] = g, x
    if fault == "drop_tail_row":      # fault: the last row of the last non-empty wave is skipped (negative tests only)
        G[n_rows - 1] = 0
    G, X = np.ascontiguousarray(G.reshape(W, rpw, m).transpose(1, 0, 2)), np.ascontiguousarray(X.reshape(W, rpw, n).transpose(1, 0, 2))
    acc, q = np.zeros((W, m, n), dt), np.zeros((W, 4, m), dt)
    step = max(1, (1 << 18) // (m * n))      # waves per pass: the accumulators of a pass stay in cache
    for w0 in range(0, W, step):
        a, tmp = acc[w0:w0 + step], np.empty_like(acc[w0:w0 + step])
        for j in range(rpw):      # one row of every wave at a time: each wave adds its products in row order
            np.multiply(G[j, w0:w0 + step, :, None], X[j, w0:w0 + step, None, :], out=tmp)
            a += tmp
    for j in range(rpw):
        q[:, j % 4] += G[j]
    if fault == "narrow_geometry":
        # fault: the partial buffer [wave][mp][pcols] has the instance's mp = 16 MB rows per wave, the combine strides through it with
        # mp = 16 ceil(m / 16) (negative tests only; differs at ceil(m / 16) in {5, 7, 8, 10, 11})
        assert m <= M_MAX and n <= N_MAX
        mp, mp_narrow, nb = 16 * mb_instance(m), 16 * ((m + 15) // 16), (n + 15) // 16
        pcols = 16 * nb + 16
        P = np.zeros((GRAM_WAVES, mp, pcols), dt)
        P[:W, :m, :n] = acc
        P[:W, :m, 16 * nb:16 * nb + 4] = q.transpose(0, 2, 1)
        R = P.reshape(-1)[:GRAM_WAVES * mp_narrow * pcols].reshape(GRAM_WAVES, mp_narrow, pcols)
        acc, q = R[:, :m, :n], R[:, :m, 16 * nb:16 * nb + 4].transpose(0, 2, 1)
    if fault == "colsum_three_quarters":      # fault: the kq = 3 slot is left out of the column sum (negative tests only)
        cs = (q[:, 0] + q[:, 1]) + q[:, 2]
    else:
        cs = (q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3])
    return _chains(acc, dt), _chains(cs, dt)


def gram(g, x, dtype=np.float64, order=None, fault=None):
    """out [m, n] = g^T x and colsum [m] = g.sum(0) in ``dtype``; .S / .n per output name in fp64.  order: "kernel" (the summation
    shape of gram.hip; the default at fp32 and with a fault) or "blas" (numpy's product; the default at fp64)."""
    dt = np.dtype(dtype)
    order = order or ("blas" if dt == np.float64 and fault is None else "kernel")
    gd, xd = np.asarray(g).astype(dt), np.asarray(x).astype(dt)
    if order == "blas":
        assert dt == np.float64 and fault is None
        out, cs = gd.T @ xd, gd.sum(0)
    else:
        out, cs = _kernel_order(dt, gd, xd, fault)
    A = lambda t: np.abs(np.asarray(t, np.float64))
    n_out, n_cs = n_terms(np.shape(g)[0])
    return types.SimpleNamespace(out=out, colsum=cs, S=dict(out=A(g).T @ A(x), colsum=A(g).sum(0)), n=dict(out=n_out, colsum=n_cs))


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# ``why`` cites the line of csrc/gram.hip (engine.py / models.py where said) the case flips.  form: "block" - G and X are column
# blocks of wider buffers, called through _lib; "step" - the views models._DenseStep.backward passes (G = dgi[:, :2d] with ldg = 3d,
# X = ws.view(n, 5, d)[:, 3] with ldx = 5d and an offset of 3d floats); "engine" - engine.gram_tn with colsum=True (tiled beyond
# 192 x 64).
_MB_LINE = {1: 169, 2: 170, 3: 171, 4: 172, 5: 173, 6: 173, 7: 174, 8: 174, 9: 174, 10: 175, 11: 175, 12: 175}
_NB_LINE = {1: 137, 2: 138, 3: 139, 4: 140}


def _case(group, kind, m, n, n_rows, why, form="block", d=None, seed=0):
    name = "%s_%dx%d_r%d" % ({"grid": "g", "rows": "r", "step": "s", "engine": "e", "normal": "n"}[group], m, n, n_rows)
    return types.SimpleNamespace(name=name, group=group, kind=kind, m=m, n=n, n_rows=n_rows, form=form, d=d, seed=seed, why=why)


def _dispatch_why(m, n):
    mb, nb = (m + 15) // 16, (n + 15) // 16
    s = "gram.hip:%d switch (mb) case %d -> MB = %d, U = %d" % (_MB_LINE[mb], mb, mb_instance(m), unroll(m))
    if mb != mb_instance(m):
        s += " (remap: partials and gram.hip:181 mp take the wider instance's geometry)"
    s += "; gram.hip:%d launch_n %s -> NB = %d" % (_NB_LINE[nb], "case %d" % nb if nb < 4 else "default", nb)
    if m % 16 or n % 16:
        s += "; m_ok / n_ok (gram.hip:47, :49) zero the lanes beyond m = %d, n = %d" % (m, n)
    return s


GRID_M = sorted({16 * k - 15 for k in range(1, 13)} | {16 * k for k in range(1, 13)})
GRID_N = sorted({16 * k - 15 for k in range(1, 5)} | {16 * k for k in range(1, 5)})
ROW_SHAPES = ((8, 64), (48, 16), (96, 32), (192, 64))       # U = 8, 4, 3, 2 (gram.hip:51)
NORMAL_SHAPES = ((1, 64), (32, 16), (80, 40), (96, 32), (120, 40), (168, 56), (192, 64))
NORMAL_ROWS = (33000, 98305)
STEP_D = (16, 40, 64)
ENGINE_SHAPES = ((193, 65), (200, 20), (30, 130), (256, 128), (384, 128))


def row_counts(m):
    u = unroll(m)
    return sorted({0, 1, 3, 4, 5, 4 * u - 1, 4 * u, 4 * u + 1, 95, 96, 97, 98303, 98304, 98305, 196613})


def _row_why(m, r):
    u = unroll(m)
    if r == 0:
        return "gram.hip:164 max(n_rows, 1): rows_per_wave = 96, every wave's range empty (gram.hip:52): all-zero out and colsum"
    if r < 4:
        return "gram.hip:57 ok = r < r_end inside the only MFMA K step: %d of 4 rows" % r
    if r in (4, 5):
        return "gram.hip:56 one K step full%s; the other U - 1 = %d steps of the iteration feed zeros" % (", one row into the next" if r == 5 else "", u - 1)
    if r in (4 * u - 1, 4 * u, 4 * u + 1):
        return "gram.hip:52 r0 += 4 U with U = %d: a tail of %d rows (%s one iteration)" % (u, r, "short of" if r < 4 * u else "exactly" if r == 4 * u else "one row past")
    if r in (95, 96, 97):
        return "gram.hip:36 r_end: wave 0's range of 96 rows %s" % ("short of a row" if r == 95 else "full" if r == 96 else "full, wave 1 holds one row")
    if r in (98303, 98304):
        return "gram.hip:164 rows_per_wave = 96 at its upper edge: all 1024 waves busy%s" % (", the last short of a row" if r == 98303 else "")
    if r == 98305:
        return "gram.hip:164 rows_per_wave steps from 96 to 192: waves 513 .. 1023 get an empty range (r_beg > n_rows), wave 512 one row"
    rpw = rows_per_wave(r)
    return "gram.hip:164 rows_per_wave = %d (a third step), the last wave's tail of %d rows is no multiple of 4 U = %d; 9 x %d < 2^24: still exact" % (
        rpw, r % rpw, 4 * u, r)


_CASE_LIST = (
    # ---- every instance and remap: 24 m x 8 n at 1000 rows (11 waves with rows, the last with 40: a tail no multiple of 4 U)
    [_case("grid", "int", m, n, 1000, _dispatch_why(m, n), seed=1000 + 7 * m + n) for m in GRID_M for n in GRID_N]
    # ---- row counts, one shape per unroll depth U
    + [_case("rows", "int", m, n, r, _row_why(m, r), seed=2000 + m + r % 1009) for m, n in ROW_SHAPES for r in row_counts(m)]
    # ---- the call forms of models._DenseStep.backward's rg_dense_train_bwd2 route
    + [_case("step", "int", 2 * d, d, 33000, "models.py:171-173 G = dgi[:, :2d] (ldg = 3d), X = ws.view(n, 5, d)[:, 3] (ldx = 5d, offset 3d); "
             + _dispatch_why(2 * d, d), form="step", d=d, seed=3000 + d) for d in STEP_D]
    # ---- engine.gram_tn's tiling
    + [_case("engine", "int", m, n, 1000, "engine.py:743-762 tiles of 192 x 64: %d x %d calls, tile copies into out / cs, colsum on the n0 == 0 "
             "tiles only (engine.py:754)" % (-(-m // 192), -(-n // 64)), form="engine", seed=4000 + m + n) for m, n in ENGINE_SHAPES]
    # ---- rounding: the widths a training step passes (m = 1: W_final through tall_linear; d = 16: 32 x 16; d = 40: 80 x 40 and
    # 120 x 40; d = 32: 96 x 32; d = 56: 168 x 56; d = 64: 192 x 64) at the row count of the existing model-level point and past the
    # rows_per_wave step
    + [_case("normal", "normal", m, n, r, "rounding at rows_per_wave = %d; " % rows_per_wave(r) + _dispatch_why(m, n), seed=5000 + m + r % 1009)
       for m, n in NORMAL_SHAPES for r in NORMAL_ROWS]
)
CASES = {c.name: c for c in _CASE_LIST}
assert len(CASES) == len(_CASE_LIST)


def inputs(case):
    """Seeded inputs of a case: g [n_rows, m], x [n_rows, n] float32."""
    rng = np.random.default_rng(case.seed)
    r, m, n = case.n_rows, case.m, case.n
    if case.kind == "int":
        return dict(g=rng.integers(-3, 4, (r, m)).astype(np.float32), x=rng.integers(-3, 4, (r, n)).astype(np.float32))
    scale = lambda k: 10.0 ** rng.uniform(np.log10(1e-3), np.log10(30.0), k)
    return dict(g=(rng.standard_normal((r, m)) * scale(m)).astype(np.float32), x=(rng.standard_normal((r, n)) * scale(n)).astype(np.float32))


def agrees(case, out, colsum, ref):
    """The comparison the GPU test applies to a result (``ref`` = exact(..) for "int" cases, gram(..) in fp64 for "normal" ones):
    bitwise equality of the values, or every element within bound(S, n, n0, C_BOUND_GRAM).  (ok out, ok colsum)."""
    if case.kind == "int":
        return bool(np.array_equal(np.asarray(out, np.float64), ref[0])), bool(np.array_equal(np.asarray(colsum, np.float64), ref[1]))
    ok = lambda v, o, n0: bool((np.abs(np.asarray(v, np.float64) - getattr(ref, o)) <= bound(ref.S[o], ref.n[o], n0, C_BOUND_GRAM)).all())
    return ok(out, "out", N0_GRAM), ok(colsum, "colsum", N0_COLSUM)
