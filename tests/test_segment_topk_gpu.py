"""rg_segment_topk alone, through engine.segment_topk, against the numpy segment_topk_ref (tests/extrap_ref.py).

Ids are compared exactly and the returned scores bit for bit; the softmax against float64 at the project's softmax tolerance
(rtol 2e-4 / atol 1e-7, test_gpu_parity.py), NaN where the float64 formula gives NaN."""
import functools

import numpy as np
import pytest
import torch

from tests import extrap_ref as R

pytestmark = pytest.mark.gpu

N_ENT = 40000
KS = (1, 10, 1024)
ALL_HIDDEN, ALL_EQUAL, ZEROS, INFS, WITH_NAN, NEG_INF = 9, 10, 11, 12, 13, 14


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _key(q):
    return q * 7 + 3


@functools.lru_cache(maxsize=None)
def _case():
    """Per query (entities, scores, known list or None = key absent from the index).  Segment lengths 0, 1 and k-1, k, k+1 for k = 1,
    10, 1024; known lists of length 0, LIST_LDS and LIST_LDS + 1, one entirely outside its segment, one covering it; the odd queries'
    pairs in shuffled entity order."""
    from red_gnn_amd import engine
    L = engine.SEGMENT_TOPK_LIST_LDS
    rng = np.random.default_rng(11)
    lengths = [0, 1, 2, 9, 10, 11, 1023, 1024, 1025, 600, 300, 200, 150, 500, 70, 2000]
    list_len = [5, None, 0, 0, 3, 20, L, L + 1, 40, 700, 40, 30, 10, 60, None, 300]
    assert {k + o for k in KS for o in (-1, 0, 1)} <= set(lengths)
    qs = []
    for q, n in enumerate(lengths):
        e = np.sort(rng.choice(N_ENT, n, replace=False))
        if q % 2:
            rng.shuffle(e)
        v = rng.standard_normal(n).astype(np.float32)
        if q % 3 == 0:
            v = np.round(v, 1)                                   # exact ties: the id decides
        if q == ALL_EQUAL:
            v[:] = 0.5                                           # the select goes through every id digit
        if q == ZEROS:
            v = rng.choice(np.array([0.0, -0.0, 1e-30, -1e-30], np.float32), n)
        if q == INFS:
            v[:5], v[5:12] = np.inf, -np.inf
        if q == NEG_INF:
            v[::7] = -np.inf
        if q == WITH_NAN:
            v[n // 3] = np.nan
        outside = np.setdiff1d(np.arange(N_ENT), e)
        k = list_len[q]
        if k is None:
            lst = None
        elif q == 5:
            lst = np.sort(rng.choice(outside, k, replace=False))                     # entirely outside the segment
        elif q == ALL_HIDDEN:
            lst = np.sort(np.concatenate([e, rng.choice(outside, k - n, replace=False)]))   # covers the whole segment
        else:
            best = e[np.argsort(-np.nan_to_num(v, nan=-9.0, posinf=9.0, neginf=-9.0), kind="stable")][:min(n, k * 2 // 3)]   # the filter bites
            lst = np.sort(np.concatenate([best, rng.choice(outside, k - len(best), replace=False)]))
        assert lst is None or (len(lst) == k and len(np.unique(lst)) == k)
        qs.append((e, v, lst))
    assert {len(l) for _, _, l in qs if l is not None} >= {0, L, L + 1}
    return qs


def _index(qs, which):
    """(keys, ptr, idx) over the lists of the queries ``which`` (sorted by key = query number)."""
    have = [q for q in sorted(set(which)) if qs[q][2] is not None]
    keys = np.array([_key(q) for q in have], np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(qs[q][2]) for q in have])]).astype(np.int64)
    idx = np.concatenate([qs[q][2] for q in have] + [np.zeros(0, np.int64)]).astype(np.int32)
    return keys, ptr, idx


def _run(qs, order, k, ptr_dtype=torch.int64, want_prob=True, use_index=True):
    """Kernel and reference on the queries ``order`` (any order, repeats allowed) as one batch."""
    from red_gnn_amd import engine
    ent = np.concatenate([qs[q][0] for q in order] + [np.zeros(0, np.int64)])
    sc = np.concatenate([qs[q][1] for q in order] + [np.zeros(0, np.float32)]).astype(np.float32)
    seg_ptr = np.concatenate([[0], np.cumsum([len(qs[q][0]) for q in order])])
    q_key = np.array([_key(q) for q in order], np.int64)
    known = _index(qs, range(len(qs))) if use_index else None
    known_dev = None if known is None else tuple(_dev(a, d) for a, d in zip(known, (torch.int64, torch.int64, torch.int32)))
    ids, val, prob = engine.segment_topk(_dev(sc, torch.float32), _dev(ent, torch.int32), _dev(seg_ptr, ptr_dtype), k,
                                         _dev(q_key, torch.int64) if use_index else None, known_dev, want_prob=want_prob)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int32 and val.dtype == torch.float32 and ids.shape == val.shape == (len(order), k)
    want = R.segment_topk_ref(sc, ent, seg_ptr, k, q_key if use_index else None, known)
    return (ids.cpu().numpy(), val.cpu().numpy(), None if prob is None else prob.cpu().numpy()), want


def _assert_equal(got, want, what):
    assert np.array_equal(got[0], want[0]), "%s: ids differ in rows %s" % (what, np.flatnonzero((got[0] != want[0]).any(1)))
    assert got[1].tobytes() == want[1].tobytes(), "%s: scores are not the input's bits" % what
    if got[2] is not None:
        assert got[2].dtype == np.float32
        np.testing.assert_allclose(got[2], want[2], rtol=2e-4, atol=1e-7, equal_nan=True, err_msg=what)


@pytest.mark.parametrize("k", KS)
def test_edges_equal_the_numpy_reference(k):
    qs = _case()
    order = list(range(len(qs)))
    got, want = _run(qs, order, k)
    _assert_equal(got, want, "k=%d" % k)
    # what the case is there for, read off the reference
    assert (want[0][ALL_HIDDEN] == -1).all() and (want[0][0] == -1).all() and want[0][1, 0] == qs[1][0][0]
    assert np.array_equal(want[0][ALL_EQUAL][:min(k, 200)], np.setdiff1d(qs[ALL_EQUAL][0], qs[ALL_EQUAL][2])[:min(k, 200)])
    assert np.array_equal(want[0][5][:min(k, 11)], _run(qs, [5], k, use_index=False)[1][0][0][:min(k, 11)])      # a list outside the segment hides nothing
    assert np.isnan(want[2][WITH_NAN][0]) and np.isnan(want[2][INFS][0]) and np.isfinite(want[2][NEG_INF][:min(k, 50)]).all()
    if k > 1:
        z = want[0][ZEROS][:2], want[1][ZEROS][:2]
        assert z[0][0] < z[0][1] and abs(z[1][0]) == abs(z[1][1]) == np.float32(1e-30) and z[1][0] > 0
        assert (want[0][:, -1] == -1).any() and (want[0][:, -1] >= 0).any() if k == 10 else True
    # int32 segment bounds, no softmax output, no index at all
    g32, _ = _run(qs, order, k, ptr_dtype=torch.int32)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(g32, got))
    gnp, _ = _run(qs, order, k, want_prob=False)
    assert gnp[2] is None and gnp[0].tobytes() == got[0].tobytes() and gnp[1].tobytes() == got[1].tobytes()
    g0, w0 = _run(qs, order, k, use_index=False)
    _assert_equal(g0, w0, "k=%d, no index" % k)
    assert not np.array_equal(w0[0], want[0])


def test_zero_signs_and_ties_follow_the_key_order():
    """-0.0 ranks equal to +0.0 (the id decides) and the returned score keeps its sign bit."""
    from red_gnn_amd import engine
    sc = np.array([-0.0, 0.0, -0.0, 0.0, -1.0], np.float32)
    ent = np.array([7, 3, 1, 9, 0], np.int32)
    ids, val, prob = engine.segment_topk(_dev(sc, torch.float32), _dev(ent, torch.int32), _dev([0, 5], torch.int32), 4)
    assert ids.cpu().tolist() == [[1, 3, 7, 9]]
    assert np.signbit(val.cpu().numpy()).tolist() == [[True, False, True, False]]
    np.testing.assert_allclose(prob.cpu().numpy(), np.full((1, 4), 1 / (4 + np.exp(-1.0))), rtol=2e-4, atol=1e-7)


@pytest.mark.parametrize("k", (10, 1024))
def test_staging_limit(k):
    """Batch 3: a segment of exactly SEGMENT_TOPK_STAGE_MAX pairs (kept in LDS), one pair more (re-read on every pass), a short one; a
    known list searched in memory, one in LDS, none; scores rounded to two decimals, so the select runs into the id digits."""
    from red_gnn_amd import engine
    S, L = engine.SEGMENT_TOPK_STAGE_MAX, engine.SEGMENT_TOPK_LIST_LDS
    rng = np.random.default_rng(5)
    qs = []
    for n, n_list in ((S, L + 44), (S + 1, L), (7, None)):
        e = rng.permutation(N_ENT)[:n]
        v = np.round(rng.standard_normal(n), 2).astype(np.float32)
        lst = None if n_list is None else np.sort(np.concatenate([e[np.argsort(-v, kind="stable")][:n_list // 2], np.setdiff1d(np.arange(N_ENT), e)[:n_list - n_list // 2]]))
        qs.append((e, v, lst))
    got, want = _run(qs, [0, 1, 2], k)
    _assert_equal(got, want, "staging, k=%d" % k)
    assert (want[0][:2] >= 0).all() and want[0][2, 6] >= 0 and want[0][2, 7] == -1
    # each of the long segments alone: its own launch, with the LDS sized for it
    for q in (0, 1):
        g, w = _run(qs, [q], k)
        _assert_equal(g, w, "staging, k=%d, query %d alone" % (k, q))
        assert all(a[0].tobytes() == b[q].tobytes() for a, b in zip(g, got))


def test_bitwise_across_runs_permutation_and_split():
    qs = _case()
    order = list(range(len(qs)))
    a, _ = _run(qs, order, 10)
    b, _ = _run(qs, order, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    perm = np.random.default_rng(2).permutation(len(qs)).tolist()
    p, want = _run(qs, perm, 10)
    _assert_equal(p, want, "permuted")
    for x, y in zip(a, p):
        assert x[perm].tobytes() == y.tobytes()
    lo, _ = _run(qs, order[:5], 10)
    hi, _ = _run(qs, order[5:], 10)
    for x, y, z in zip(a, lo, hi):
        assert x.tobytes() == np.concatenate([y, z]).tobytes()


def test_segment_bounds_are_clamped_and_arguments_checked():
    from red_gnn_amd import _lib, engine
    rng = np.random.default_rng(3)
    sc, ent = rng.standard_normal(50).astype(np.float32), rng.permutation(500)[:50].astype(np.int32)
    ids, val, prob = engine.segment_topk(_dev(sc, torch.float32), _dev(ent, torch.int32), _dev([-5, 20, 10, 10 ** 6], torch.int64), 10)
    torch.cuda.synchronize()
    want = R.segment_topk_ref(sc, ent, [-5, 20, 10, 10 ** 6], 10)    # [-5, 20) -> [0, 20); [20, 10) -> empty; [10, 10^6) -> [10, 50)
    assert (want[0][1] == -1).all() and (want[0][[0, 2]] >= 0).all()
    _assert_equal((ids.cpu().numpy(), val.cpu().numpy(), prob.cpu().numpy()), want, "clamped bounds")
    for k in (0, 1025):
        with pytest.raises(_lib.NativeError):
            engine.segment_topk(_dev(sc, torch.float32), _dev(ent, torch.int32), _dev([0, 50], torch.int64), k)
