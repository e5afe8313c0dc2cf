"""tests/saliency_ref.py on its own (no GPU): at fp64 it is tests/rescore_ref.rescore (1e-12) on every case with and without the case's
deletion mask; its autograd gradient agrees with central finite differences of its own forward on every live edge; dead edges and
unreached rows get exactly 0."""
import numpy as np
import pytest
import torch

from tests import rescore_ref as R
from tests import saliency_ref as S

TOL = 1e-12
_CACHE = {}


def _case(name):
    if name not in _CACHE:
        c = R.make_case(name, **R.CASES[name])
        c.keep = ~R.fact_mask(c.edges, c.n_rel, c.facts, c.fact_rows)
        c.args = (c.params, c.edges, c.subs, c.rels, c.n_ent, c.L, c.act)
        c.sal = {None: S.saliency(*c.args), "mask": S.saliency(*c.args, keep=c.keep)}
        _CACHE[name] = c
    return _CACHE[name]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", list(R.CASES))
def test_fp64_reproduces_rescore_ref(name, masked):
    c = _case(name)
    keep = c.keep if masked else None
    score, reached, live, alpha, grad = c.sal["mask" if masked else None]
    w_score, w_reached, w_live, w_alpha = R.rescore(*c.args, keep=keep)
    assert np.array_equal(reached, w_reached) and np.array_equal(live, w_live)
    print("%s masked=%s: max |score - rescore_ref| %.3g, |alpha - ...| %.3g" % (name, masked, np.abs(score - w_score).max(),
                                                                                  np.abs(alpha - w_alpha).max()))
    assert np.abs(score - w_score).max() <= TOL and np.abs(alpha - w_alpha).max() <= TOL
    # dead edges and rows that are not reached: exactly 0
    assert (grad[~live] == 0).all() and (grad[~reached[c.edges[:, 0]]] == 0).all() and (score[~reached] == 0).all()
    if masked:
        assert (~reached).any() and 4 * reached.sum() >= c.B
    assert np.abs(grad[live & reached[c.edges[:, 0]]]).max() > 0


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("name", ["e300_L2", "e300_L3"])
def test_autograd_agrees_with_central_differences_on_every_live_edge(name, masked):
    c = _case(name)
    keep = c.keep if masked else None
    score, reached, live, alpha, grad = c.sal["mask" if masked else None]
    fd = S.finite_differences(*c.args, keep, live, step=1e-6)
    row = c.edges[:, 0]
    scale = np.zeros(c.B)
    np.maximum.at(scale, row, np.abs(grad))
    err = np.abs(fd - grad)
    worst = (err[live] / np.maximum(scale[row[live]], 1e-300)).max()
    print("%s masked=%s: %d live edges, max |fd - autograd| / max |grad of the row| %.3g" % (name, masked, live.sum(), worst))
    assert (err[live] <= 1e-6 * scale[row[live]]).all()


def test_fp32_reference_is_close_to_fp64():
    c = _case("e300_L3")
    g64 = c.sal["mask"][4]
    s32, _, live32, _, g32 = S.saliency(*c.args, keep=c.keep, dtype=torch.float32)
    assert s32.dtype == np.float32 and g32.dtype == np.float32 and np.array_equal(live32, c.sal["mask"][2])
    assert np.abs(g32 - g64).max() <= 1e-4 * max(1.0, np.abs(g64).max()) and np.array_equal(g32 == 0, g64 == 0)


def test_first_order_estimate_of_a_deletion():
    """score - sum of the deleted live edges' gradients is the tangent's estimate of the rescore: exact to second order, so it beats
    'no change' on most rows the deletion leaves reached."""
    c = _case("e300_L2")
    score, reached, live, alpha, grad = c.sal[None]
    after = c.sal["mask"]
    est = score - np.bincount(c.edges[:, 0], weights=np.where(~c.keep, grad, 0.0), minlength=c.B)
    rows = after[1]
    assert np.isfinite(est).all() and rows.any()
    print("e300_L2: |estimate - rescore| %s, |score - rescore| %s" % (np.abs(est - after[0])[rows].round(4), np.abs(score - after[0])[rows].round(4)))
