"""The attention-profile kernels called on their own - engine.attn_profile, tattn_profile, xattn_profile, i.e. csrc/profile.hip's
rg_attn_profile / rg_tattn_profile / rg_xattn_profile - against tests/hop_ref.py, over its case table: layer_ref's dispatch cases, the
B = 1024 cases that put profile_hop's words per wave step at 8, 16, 32 and 64, and the windowed case on the 64 - 80 KiB LDS launch.
Setup as tests/test_explain_kernels_gpu.py (frontier expanded hop by hop, node lists equal to the oracle's).  Per hop:

  1. count equals the bincount of the oracle's hop over (query, [direction | lag bin,] relation) in every cell
  2. sum equals hop_ref.expected_profile of the DEVICE's alphas - explain_hop with every node marked and tau = 0 - as int64, exactly:
     the two kernels' alphas are the same bits (and test_explain_kernels_gpu.py ties those to the layer forward's).  Separately
     |sum 2^-32 - sum of alpha64| <= sum of the per-edge bounds (hop_ref.alpha_bound) + count 2^-33 per cell
  3. the outputs accumulate: on a random non-negative base the result is base + expected, a second call adds the same again, cells
     without edges keep their base
  4. temporal: all three directions occur
  5. extrapolation: the identity lag table (n_bins = n_tab), the all-zero table (n_bins = 1), and a table with one occurring entry
     >= n_bins, whose edges vanish from both outputs while nothing else changes
  6. invariance (hop_ref.SMALL and gw16): the two halves of a batch, each on a frontier of its own, give the halves of the whole; a
     permutation of the queries permutes the rows
"""

import time

import numpy as np
import pytest
import torch

from tests import hop_ref as hr
from tests.test_explain_kernels_gpu import device_alphas, sub_batch, sub_tables, walk
from tests.test_layer_kernels_gpu import _dev, _extra

pytestmark = pytest.mark.gpu

# worst |sum 2^-32 - sum of alpha64| / (sum of the per-edge bounds + count 2^-33) per entry point over the cells of the table, as measured
# on an MI355X (information only; the assertion is the bound itself, i.e. 1).  The figures near 0.6 are cells of one or two edges with
# alpha ~ 1e-7 .. 1e-6, where the per-edge bound is below 2^-33 and the rounding to 2^-32 is all of the error: numpy's fp32 alphas give
# the same 0.607 (ap_32 hop 1) and 0.617 (x_lds80 hop 1)
KERNEL_RATIOS = {"rg_attn_profile": 0.607, "rg_tattn_profile": 0.0764, "rg_xattn_profile": 0.617}
# wall time of this file on an MI355X: 4.3 s (28 tests, 1.3 s of it inside the tests; the slowest, tickets, 0.4 s)


def profile(case, fr, g, level, X, ex, sum_out, count_out, lag=None):
    """One call of the case's profile entry point; ``lag`` = (uint8 table, n_bins) for the windowed kind."""
    from red_gnn_amd import engine as eng
    attn = (X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], case.attn_dim, sum_out, count_out)
    if case.kind == "static":
        eng.attn_profile(fr, g, level, *attn)
    elif case.kind == "temporal":
        eng.tattn_profile(fr, g, level, ex["q_time"], *attn)
    else:
        eng.xattn_profile(fr, g, level, ex["q_time"], ex["loop_time"], ex["row_time"], _dev(lag[0], torch.uint8), lag[1], *attn)
    torch.cuda.synchronize()


def _run(case, fr, g, level, X, ex, shape, lag=None, base=None, calls=1):
    """(sum, count) as numpy after ``calls`` calls on outputs that start from ``base`` = (sum, count) or zero."""
    out = [torch.zeros(shape, dtype=torch.int64, device="cuda") if base is None else _dev(b, torch.int64) for b in (base or (None, None))]
    for _ in range(calls):
        profile(case, fr, g, level, X, ex, out[0], out[1], lag)
    return out[0].cpu().numpy(), out[1].cpu().numpy()


def _lag_tables(case, hop):
    """[(what, table, n_bins)] of step 5; [(.., None, None)] for the other kinds."""
    if case.kind != "windowed":
        return [("", None, None)]
    ident = np.arange(case.n_tab, dtype=np.uint8)
    hit = int(np.bincount(hop.trow, minlength=case.n_tab).argmax())      # the time-table row most edges have
    holed = ident.copy()
    holed[hit] = 200
    return [("identity table", ident, case.n_tab), ("zero table", np.zeros(case.n_tab, np.uint8), 1), ("row %d outside the bins" % hit, holed, case.n_tab)]


@pytest.mark.parametrize("name", list(hr.CASES))
def test_profile_vs_reference(name):
    t0 = time.time()
    rng = np.random.default_rng(11)
    dirs = np.zeros(3, np.int64)
    records = []

    def after():      # ---- 6.
        if name in hr.SMALL or name == "gw16":
            _invariance(records, rng)
    for h in walk(name, after):
        case, tag, hop = h.case, h.tag, h.hop
        B, R = case.B, case.n_rela_rows
        got, _, tab = device_alphas(h)
        assert len(got.edges) == hop.E, tag
        alpha_dev = tab.at(h.edges[:, 0], h.edges[:, 1], h.edges[:, 2])      # the device's alphas in the oracle's edge order
        assert alpha_dev.dtype == np.float32
        a64, kap, bnd = hr.alpha_ref(case, hop, h.x)
        results = {}
        for what, table, n_bins in _lag_tables(case, hop):
            lag = None if table is None else (table, n_bins)
            shape, cell = hr.profile_cells(hop, B, R, case.kind, table, n_bins)
            want_sum, want_count = hr.expected_profile(hop, alpha_dev, B, R, case.kind, table, n_bins)
            s, c = _run(case, h.fr, h.g, h.level, h.X, h.ex, shape, lag)
            # ---- 1. counts, 2. sums
            assert np.array_equal(c, want_count), "%s %s: %d cells with another count" % (tag, what, int((c != want_count).sum()))
            diff = np.abs(s - want_sum)
            assert not diff.any(), ("%s %s: %d cells whose sum is not the sum of explain's alphas; largest difference %d units of 2^-32"
                                    % (tag, what, int((diff > 0).sum()), int(diff.max())))
            err = np.abs(s.astype(np.float64) / hr.SCALE - hr.cell_sums(shape, cell, a64))
            allowed = hr.cell_sums(shape, cell, bnd) + want_count * hr.Q
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.where(want_count > 0, err / allowed, 0.0).max())
            print("%s %s (E %d, cells with edges %d): sum worst ratio %.3g" % (tag, what, int(want_count.sum()), int((want_count > 0).sum()), ratio))
            assert (err <= allowed).all(), "%s %s: sum beyond the fp64 bound, worst ratio %.3g" % (tag, what, ratio)
            # ---- 3. accumulation
            base = (rng.integers(0, 1 << 40, shape), rng.integers(0, 1 << 20, shape))
            for calls in (1, 2):
                s2, c2 = _run(case, h.fr, h.g, h.level, h.X, h.ex, shape, lag, base, calls)
                assert np.array_equal(s2, base[0] + calls * want_sum) and np.array_equal(c2, base[1] + calls * want_count), (tag, what, calls)
                assert np.array_equal(s2[want_count == 0], base[0][want_count == 0]), (tag, what, calls)
            results[what] = (s, c)
        if case.kind == "temporal":
            dirs += results[""][1].sum((0, 2))
        if case.kind == "windowed":
            # ---- 5. the dropped entry: its bin is empty, every other cell is the identity table's; the zero table is the sum over bins
            (s_id, c_id), (s_0, c_0), (s_h, c_h) = results.values()
            hit = int(np.bincount(hop.trow, minlength=case.n_tab).argmax())
            assert c_id[:, hit].sum() > 0 and not c_h[:, hit].any() and not s_h[:, hit].any(), tag
            keep = np.arange(case.n_tab) != hit
            assert np.array_equal(c_h[:, keep], c_id[:, keep]) and np.array_equal(s_h[:, keep], s_id[:, keep]), tag
            assert np.array_equal(c_0[:, 0], c_id.sum(1)) and np.array_equal(s_0[:, 0], s_id.sum(1)), tag
        records.append((h, results))
    if records[0][0].case.kind == "temporal":
        print("%s: edges per direction %s" % (name, dirs.tolist()))
        if name == "temporal":
            assert (dirs > 0).all(), dirs      # ---- 4.
    print("%s: %.2f s" % (name, time.time() - t0))


def _invariance(records, rng):
    """Step 6 on the first lag table of every hop."""
    case, g = records[0][0].case, records[0][0].g
    B = case.B
    if B < 2:
        return
    perm = rng.permutation(B)
    cut = B // 2 + 1
    for rows in (np.arange(cut), np.arange(cut, B), perm):
        one, fr = sub_batch(case, rows)
        ex = _extra(one)
        for h, results in records:
            fr.expand(g)
            what, table, n_bins = _lag_tables(case, h.hop)[0]
            whole_s, whole_c = results[what]
            shape = (len(rows),) + whole_s.shape[1:]
            s, c = _run(one, fr, g, h.level, sub_tables(h, rows), ex, shape, None if table is None else (table, n_bins))
            assert np.array_equal(c, whole_c[rows]) and np.array_equal(s, whole_s[rows]), "%s: queries %s.. on a frontier of their own" % (h.tag, rows[:3])
        fr.close()
