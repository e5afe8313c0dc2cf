"""tests/tsaliency_ref.py on its own (no GPU), for both temporal models: at fp64 and gate = 1 it is tests/trescore_ref.rescore /
tests/xrescore_ref.rescore on their cases with and without the case's deletion mask; its autograd gradient agrees with central
differences of its own forward in the gates; dead edges and unreached rows get exactly 0.

The two references add a node's edges in different orders (numpy's add.at, torch's index_add), so their fp64 values differ by a few
units of 2^-53 of the value: 1e-12 is taken of max(1, |value|).  The extrapolation cases with relu reach scores of some 10^4, where
1e-12 absolute would be less than one unit in the last place (measured there: 7.3e-12 where the largest |score| is 2.5e4, 2.3e-12 at 1.1e3;
at most 7.2e-15 on the interpolation cases, whose scores stay below 10).

The central differences use a step of 1e-6 on scores of order 1, so they carry a rounding error of about 2^-53 / 1e-6 = 1e-10
themselves: an edge passes within 1e-6 of the largest |gradient| of its row, that scale taken as at least 1e-3 (a row of a
saturated tanh has gradients of 1e-7)."""
import numpy as np
import pytest
import torch

from tests import extrap_ref as XR
from tests import trescore_ref as TR_
from tests import tsaliency_ref as S
from tests import xrescore_ref as XR_
from tests.test_trescore_ref import CASES as T_CASES, N_ENT as T_N_ENT, _case as _t_case
from tests.test_xrescore_ref import CASES as X_CASES, _case as _x_case

TOL = 1e-12
FD_EDGES = 48                                            # live edges per row moved by the central differences (the first ones)
_CACHE = {}


def _temporal(L, shared, act):
    key = ("t", L, shared, act)
    if key not in _CACHE:
        c = _t_case(L, shared, act)
        args = ("temporal", c["p"], c["edges"], c["etime"], c["times"], c["heads"], c["rels"], T_N_ENT, L, act)
        ref = lambda keep: TR_.rescore(c["p"], c["edges"], c["etime"], c["heads"], c["rels"], c["times"], T_N_ENT, L, act, keep=keep,
                                       shared_tables=shared)
        _CACHE[key] = (args, dict(shared_tables=shared), ~c["mask"], ref, c["edges"])
    return _CACHE[key]


def _extrapolation(d, a, act, L, B):
    key = ("x", d, a, act, L, B)
    if key not in _CACHE:
        data, q, p, logits, last, cur_t, q_of, objs, edges, data_row, day, reached = _x_case(d, a, act, L, B)
        heads, rels, q_day = q[q_of, 0], q[q_of, 1], cur_t[q_of]
        keep = ~XR_.fact_mask(edges, day, data_row, XR.N_REL, XR_.deleted_facts(data, edges, data_row, day, heads))
        args = ("extrapolation", p, edges, day, q_day, heads, rels, XR.N_ENT, L, act)
        ref = lambda keep: XR_.rescore(p, edges, day, q_day, heads, rels, XR.N_ENT, L, act, keep=keep)
        _CACHE[key] = (args, {}, keep, ref, edges)
    return _CACHE[key]


def _all_cases():
    return [("t",) + c for c in T_CASES] + [("x",) + c for c in X_CASES]


def _get(case):
    return _temporal(*case[1:]) if case[0] == "t" else _extrapolation(*case[1:])


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", _all_cases(), ids=lambda c: "-".join(map(str, c)))
def test_fp64_at_gate_one_reproduces_the_rescore_reference(case, masked):
    args, kw, keep, ref, edges = _get(case)
    keep = keep if masked else None
    score, reached, live, alpha, grad = S.saliency(*args, keep=keep, **kw)
    w_score, w_reached, w_live, w_alpha = ref(keep)
    assert np.array_equal(reached, w_reached) and np.array_equal(live, w_live)
    print("%s masked=%s: E %d, max |score - rescore ref| %.3g (largest |score| %.3g), |alpha - ...| %.3g"
          % (case, masked, len(edges), np.abs(score - w_score).max(), np.abs(w_score).max(), np.abs(alpha - w_alpha).max()))
    assert (np.abs(score - w_score) <= TOL * np.maximum(1.0, np.abs(w_score))).all() and np.abs(alpha - w_alpha).max() <= TOL
    # dead edges and rows that are not reached: exactly 0
    assert (grad[~live] == 0).all() and (grad[~reached[edges[:, 0]]] == 0).all() and (score[~reached] == 0).all()
    if masked:                                            # the condition of the deletion mask, with the reference alone
        assert (ref(None)[1] & ~reached).any() and 4 * reached.sum() >= len(reached)
    assert np.abs(grad[live & reached[edges[:, 0]]]).max() > 0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", [("t", 2, False, "relu"), ("t", 3, False, "tanh"), ("x", 20, 3, "idd", 2, 3), ("x", 32, 5, "tanh", 3, 9)],
                         ids=lambda c: "-".join(map(str, c)))
def test_autograd_agrees_with_central_differences(case, masked):
    args, kw, keep, ref, edges = _get(case)
    keep = keep if masked else None
    score, reached, live, alpha, grad = S.saliency(*args, keep=keep, **kw)
    fd = S.finite_differences(*args, keep, live, step=1e-6, most=FD_EDGES, **kw)
    moved = live & ~np.isnan(fd)
    row = edges[:, 0]
    scale = np.zeros(len(reached))
    np.maximum.at(scale, row, np.abs(grad))
    err = np.abs(fd - grad)
    worst = (err[moved] / np.maximum(scale[row[moved]], 1e-300)).max()
    print("%s masked=%s: %d of %d live edges moved, max |fd - autograd| / max |grad of the row| %.3g" % (case, masked, moved.sum(), live.sum(), worst))
    assert moved.sum() >= min(live.sum(), 100) and (err[moved] <= 1e-6 * np.maximum(scale[row[moved]], 1e-3)).all()


def test_fp32_reference_is_close_to_fp64():
    for case in (("t", 3, False, "tanh"), ("x", 32, 5, "tanh", 3, 9)):
        args, kw, keep, ref, edges = _get(case)
        g64 = S.saliency(*args, keep=keep, **kw)
        s32, _, live32, _, g32 = S.saliency(*args, keep=keep, dtype=torch.float32, **kw)
        assert s32.dtype == np.float32 and g32.dtype == np.float32 and np.array_equal(live32, g64[2])
        assert np.abs(g32 - g64[4]).max() <= 1e-4 * max(1.0, np.abs(g64[4]).max())
