"""The extrapolation attention profile without a GPU: the lag bins, AttentionProfile with a lag axis on CPU tensors, and the float64
reference of the GPU tests (tests/extrap_profile_ref.py) against tests/profile_ref.py's group-by of the same hops."""
import numpy as np
import pytest
import torch

from red_gnn_amd import _lib
from red_gnn_amd import profile as P
from tests import extrap_profile_ref as XP
from tests import extrap_ref as R
from tests import profile_ref as PR


def test_check_lag_edges():
    assert P.DEFAULT_LAG_EDGES == (2, 4, 8, 15, 31, 61, 121)
    assert P.check_lag_edges(P.DEFAULT_LAG_EDGES) == P.DEFAULT_LAG_EDGES
    assert P.check_lag_edges(()) == () and P.check_lag_edges([0]) == (0,)
    assert P.check_lag_edges(np.array([1, 5, 9])) == (1, 5, 9) and P.check_lag_edges(range(1, 256)) == tuple(range(1, 256))
    assert all(type(e) is int for e in P.check_lag_edges(np.array([1, 5, 9])))
    for bad in ([2, 2], [3, 2], [-1, 2], [1.5], [True], ["1"], range(256), 7, None, [[1, 2]]):
        with pytest.raises(ValueError):
            P.check_lag_edges(bad)


def test_lag_bins():
    assert P.lag_bins(np.array([0, 1, 2, 120, 121, 500]), P.DEFAULT_LAG_EDGES).tolist() == [0, 0, 1, 6, 7, 7]
    assert P.lag_bins(np.array([0, 1, 2, 120, 121, 500]), ()).tolist() == [0] * 6
    assert P.lag_bins(np.arange(5), (0, 3)).tolist() == [1, 1, 1, 2, 2]                  # a first edge of 0: bin 0 stays empty
    assert int(P.lag_bins(3, (2, 4))) == 1


def _lag_profile(seed=0, G=3, L=2, n_bins=8, R_=5, edges=P.DEFAULT_LAG_EDGES):
    g = torch.Generator().manual_seed(seed)
    count = torch.randint(0, 4, (G, L, n_bins, R_), generator=g)
    fixed = count * torch.randint(1, 2 ** 32, (G, L, n_bins, R_), generator=g)
    return P.AttentionProfile(fixed, count, "query", ("group", "hop", "lag", "relation"), edges)


def test_profile_with_a_lag_axis():
    p = _lag_profile()
    c = p.collapse("lag")
    assert c.axes == ("group", "hop", "relation") and c.lag_edges is None
    assert torch.equal(c.count, p.count.sum(2)) and torch.equal(c.fixed, p.fixed.sum(2))
    with pytest.raises(ValueError):
        c.collapse("lag")
    t = p.total()
    assert t.lag_edges == p.lag_edges and t.axes == p.axes and torch.equal(t.count, p.count.sum(1, keepdim=True))
    assert p.cpu().lag_edges == p.lag_edges
    # top: all bins = the collapsed profile's; one bin = that slice's
    ids, mean = p.top(1, k=3)
    ids_c, mean_c = c.top(1, k=3)
    assert torch.equal(ids, ids_c) and torch.allclose(mean, mean_c, rtol=0, atol=0, equal_nan=True)
    ids5, mean5 = p.top(1, k=3, lag=5)
    want = P.AttentionProfile(p.fixed[:, :, 5], p.count[:, :, 5], "query").top(1, k=3)
    assert torch.equal(ids5, want[0]) and torch.allclose(mean5, want[1], equal_nan=True)
    for bad in (8, -1, True, 1.0):
        with pytest.raises(ValueError):
            p.top(1, k=3, lag=bad)
    with pytest.raises(ValueError):
        p.top(1, k=3, direction=0)                                      # no direction axis on a lag profile
    with pytest.raises(ValueError):
        c.top(1, k=3, lag=0)                                            # no lag axis left
    d = P.AttentionProfile(p.fixed[:, :, :3], p.count[:, :, :3], "query", ("group", "hop", "direction", "relation"))
    with pytest.raises(ValueError):
        d.top(1, lag=0)
    assert d.lag_edges is None and d.collapse("direction").lag_edges is None
    # labels
    assert p.lag_labels() == [(0, 1), (2, 3), (4, 7), (8, 14), (15, 30), (31, 60), (61, 120), (121, None)]
    assert _lag_profile(n_bins=1, edges=()).lag_labels() == [(0, None)]
    for q in (c, d):
        with pytest.raises(ValueError):
            q.lag_labels()
        with pytest.raises(ValueError):
            q.lag_share(0)


def test_lag_share():
    p = _lag_profile(seed=1)
    p.count[2, 1] = 0
    p.fixed[2, 1] = 0
    for row in range(3):
        s = p.lag_share(row)
        assert s.dtype == torch.float64 and tuple(s.shape) == (2, 8)
        mass = p.fixed[row].sum(-1).double()
        for l in range(2):
            if p.count[row, l].sum() == 0:
                assert torch.isnan(s[l]).all()
            else:
                assert torch.allclose(s[l], mass[l] / mass[l].sum(), rtol=1e-15, atol=0) and abs(float(s[l].sum()) - 1.0) < 1e-12
    assert torch.isnan(p.lag_share(2)[1]).all() and not torch.isnan(p.lag_share(2)[0]).any()
    with pytest.raises(ValueError):
        p.lag_share(3)


def test_profiles_add_only_with_equal_edges():
    p, q = _lag_profile(seed=2), _lag_profile(seed=3)
    s = p + q
    assert s.lag_edges == p.lag_edges and torch.equal(s.count, p.count + q.count) and torch.equal(s.fixed, p.fixed + q.fixed)
    other = _lag_profile(seed=3, edges=(1, 2, 3, 4, 5, 6, 7))
    with pytest.raises(ValueError):
        p + other
    with pytest.raises(ValueError):
        p + P.AttentionProfile(q.fixed, q.count, "query", q.axes)        # edges missing
    # the existing positional constructor calls still work and add
    a = P.AttentionProfile(p.fixed[:, :, 0], p.count[:, :, 0], "query", ("group", "hop", "relation"))
    assert (a + a).lag_edges is None and a.lag_edges is None


@pytest.mark.parametrize("d,a,act,n_layer,B", R.CASES[:1] + R.CASES[2:])
def test_reference_cells_sum_to_the_relation_profile(d, a, act, n_layer, B):
    from oracle import redgnn_oracle as orc
    from tests.test_extrap_ref import _state
    data, q = R.make_case(d, B)
    off = orc.get_time_offset_list(data, 24)
    _, _, hops, cur_t = R.walk(_state(d, a, n_layer), data, off, 24, R.N_ENT, R.N_REL, q[:, 0], q[:, 1], q[:, 3], n_layer, act)
    n_rows = R.N_REL + 2
    count, asum = XP.profile_cells(hops, cur_t, B, n_rows, P.DEFAULT_LAG_EDGES)
    assert count.shape == (B, n_layer, 8, n_rows) and count.dtype == np.int64 and asum.dtype == np.float64
    c_ref, s_ref = PR.profile_by_query([h[0] for h in hops], [h[1] for h in hops], B, n_rows)
    assert np.array_equal(count.sum(2), c_ref)
    np.testing.assert_allclose(asum.sum(2), s_ref, rtol=1e-12, atol=1e-12)
    cr, sr = PR.by_relation(count.sum(2), asum.sum(2), q[:, 1], n_rows)
    cr_ref, sr_ref = PR.by_relation(c_ref, s_ref, q[:, 1], n_rows)
    assert np.array_equal(cr, cr_ref)
    np.testing.assert_allclose(sr, sr_ref, rtol=1e-12, atol=1e-12)
    # one bin per day refines the default bins; one bin is the collapsed table
    fine_c, fine_s = XP.profile_cells(hops, cur_t, B, n_rows, tuple(range(1, 250)))
    fold = P.lag_bins(np.arange(250), P.DEFAULT_LAG_EDGES)
    folded = np.zeros_like(count)
    np.add.at(folded, (slice(None), slice(None), fold), fine_c)
    assert np.array_equal(folded, count)
    assert np.array_equal(XP.profile_cells(hops, cur_t, B, n_rows, ())[0][:, :, 0], c_ref)
    # every self-loop sits in the self-loop relation's column, at the lag of the window's first day
    loops = sum(int((h[0][:, 4] < 0).sum()) for h in hops)
    assert count[..., R.N_REL].sum() == loops and count[..., R.N_REL + 1].sum() == 0


def test_the_symbol_is_declared():
    assert "rg_xattn_profile" in _lib.SYMBOLS
