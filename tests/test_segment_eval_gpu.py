"""rg_segment_eval on the GPU against tests/segment_eval_ref.py, which builds every query's dense fp32 row and works from it.

The counts and ``visited`` are integers and compared exactly.  ``logp`` is compared with the project's stated tolerance (README: rtol
1e-4, atol 2e-5) against the float64 value computed from the same fp32 logits; NaN where the reference has NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import segment_eval_ref as R

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _index_dev(ix):
    return None if ix is None else tuple(_dev(a, d) for a, d in zip(ix, (torch.int64, torch.int64, torch.int32)))


def _run(scores, ent, seg_ptr, target, n_ent, key_a=None, index_a=None, key_b=None, index_b=None, ptr_dtype=torch.int64):
    from red_gnn_amd import engine
    out = engine.segment_eval(_dev(scores, torch.float32), _dev(ent, torch.int32), _dev(seg_ptr, ptr_dtype), _dev(target, torch.int32), n_ent,
                              None if index_a is None else _dev(key_a, torch.int64), _index_dev(index_a),
                              None if index_b is None else _dev(key_b, torch.int64), _index_dev(index_b))
    torch.cuda.synchronize()
    logp, counts, visited = (x.cpu() for x in out)
    assert logp.dtype == torch.float32 and counts.dtype == torch.int32 and visited.dtype == torch.int32
    assert logp.shape == visited.shape == (len(target),) and counts.shape == (len(target), 6)
    return logp.numpy(), counts.numpy().astype(np.int64), visited.numpy() != 0


def _run_case(c, qs, **kw):
    """The queries ``qs`` of the edge case in the order given, their pairs laid out in that order."""
    sp = c["seg_ptr"]
    pairs = np.concatenate([np.arange(sp[q], sp[q + 1]) for q in qs] + [np.zeros(0, np.int64)]).astype(np.int64)
    seg_ptr = np.concatenate([[0], np.cumsum([sp[q + 1] - sp[q] for q in qs])])
    return _run(c["scores"][pairs], c["ent"][pairs], seg_ptr, c["target"][qs], R.N_ENT, c["key_a"][qs], c["index_a"], c["key_b"][qs],
                c["index_b"], **kw)


def _assert_same(got, want, what):
    logp, counts, visited = got
    w_logp, w_counts, w_visited = want
    assert np.array_equal(counts, w_counts), "%s: counts differ at queries %s:\n%s\nvs\n%s" % (
        what, np.flatnonzero((counts != w_counts).any(1)), counts[(counts != w_counts).any(1)], w_counts[(counts != w_counts).any(1)])
    assert np.array_equal(visited, w_visited), what
    assert np.array_equal(np.isnan(logp), np.isnan(w_logp)), what
    ok = ~np.isnan(w_logp)
    err = np.abs(logp[ok] - w_logp[ok])
    print("%s: max |logp - ref| = %.3g" % (what, err.max() if ok.any() else 0.0))
    assert np.all(err <= ATOL + RTOL * np.abs(w_logp[ok])), "%s: logp %s vs %s" % (what, logp, w_logp)


def test_edge_case_equals_the_dense_reference():
    """One call over the 22 segments of segment_eval_ref.edge_case (see LENGTHS, A_LEN, B_LEN there); then with int32 bounds, without
    the first index (n_keys = 0 with NULL arrays) and with an empty one."""
    c = R.edge_case()
    qs = np.arange(len(R.LENGTHS))
    want = c["ref"]
    assert np.isnan(want[0][R.WITH_NAN]) and not want[2][0] and want[2].sum() == 16
    _assert_same(_run_case(c, qs), want, "one call")
    _assert_same(_run_case(c, qs, ptr_dtype=torch.int32), want, "one call, int32 bounds")
    no_a = (want[0], np.concatenate([want[1][:, :2], want[1][:, :2], want[1][:, 4:]], 1), want[2])       # nothing to filter: the raw counts
    _assert_same(_run_case(dict(c, index_a=None), qs), no_a, "no first index")
    empty = (np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros(0, np.int32))
    _assert_same(_run_case(dict(c, index_a=empty), qs), no_a, "empty first index")
    no_b = (want[0], np.concatenate([want[1][:, :4], want[1][:, :2]], 1), want[2])
    _assert_same(_run_case(dict(c, index_b=None), qs), no_b, "no second index")


def test_full_row_has_no_implicit_zero():
    """n_ent = 300 and segments of all 300 entities, every score negative: a kernel that lets a zero into the maximum, the sum or the
    counts shows (logp would be off by about log(1 + 300 e^-m), gt by one or more).  The second query is the first shifted to about
    -200: there exp(-m) overflows fp32, so a zeros' term formed as 0 * exp(-m) would turn a finite logp into NaN."""
    rng = np.random.default_rng(8)
    n_ent = 300
    ent = rng.permutation(n_ent)
    base = (-np.abs(rng.standard_normal(n_ent)) * 3 - 0.5).astype(np.float32)
    base[5] = base[17]                                           # one exact tie with the target
    scores = np.concatenate([base, base - np.float32(200)])
    assert scores[n_ent:].max() < -150 and scores[n_ent + 5] == scores[n_ent + 17]
    ents = np.concatenate([ent, ent])
    target = np.array([ent[17], ent[17]])
    seg_ptr = np.array([0, n_ent, 2 * n_ent])
    listed = (np.array([4], np.int64), np.array([0, 3], np.int64), np.sort(np.array([ent[5], ent[int(np.argmax(base))], n_ent + 1])).astype(np.int32))
    key_a, key_b = np.array([4, 4]), np.array([9, 9])            # the second index lacks key 9
    want = R.segment_eval(scores, ents, seg_ptr, target, n_ent, key_a, listed, key_b, listed)
    for q in range(2):
        c = want[1][q]
        assert c[1] == 1 and c[3] == 0 and c[2] < c[0] and np.array_equal(c[4:], c[:2]) and np.isfinite(want[0][q])
    assert np.array_equal(want[1][0], want[1][1]) and abs(want[0][0] - want[0][1]) < 1e-3      # (the shift rounds the scores)
    _assert_same(_run(scores, ents, seg_ptr, target, n_ent, key_a, listed, key_b, listed), want, "full rows")
    ex = np.exp(base.astype(np.float64))                         # the softmax over the 300 scores alone
    assert abs(want[0][0] - np.log(ex[17] / ex.sum() + 1e-12)) < 1e-12


def test_results_do_not_depend_on_the_batch():
    """Reversed query order, and every query alone at batch = 1: logp bitwise equal and the counts equal, per query."""
    c = R.edge_case()
    qs = np.arange(len(R.LENGTHS))
    whole = _run_case(c, qs)
    rev = _run_case(c, qs[::-1].copy())
    for w, r in zip(whole, rev):
        assert w.tobytes() == r[::-1].tobytes()
    for q in qs:
        one = _run_case(c, np.array([q]), ptr_dtype=torch.int32)
        for w, o in zip(whole, one):
            assert w[q:q + 1].tobytes() == o.tobytes(), "B = 1, query %d" % q


def test_argument_errors_launch_nothing():
    from red_gnn_amd import _lib
    L = _lib.lib()
    c = R.edge_case()
    B = 3
    scores, ent = _dev(c["scores"][:3], torch.float32), _dev(c["ent"][:3], torch.int32)
    seg_ptr, target = _dev([0, 1, 3, 3], torch.int64), _dev(c["target"][1:4], torch.int32)
    keys = _dev(c["key_a"][:B], torch.int64)
    logp = torch.full((B,), -7.0, device="cuda")
    counts = torch.full((B, 6), -7, dtype=torch.int32, device="cuda")
    visited = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    p = _lib.ptr

    def call(batch=B, n_ent=R.N_ENT, a=(None, None, None, None, 0), b=(None, None, None, None, 0)):
        return L.rg_segment_eval(p(scores), p(ent), 3, p(seg_ptr), 1, p(target), batch, n_ent, p(a[0]), p(a[1]), p(a[2]), p(a[3]), a[4],
                                 p(b[0]), p(b[1]), p(b[2]), p(b[3]), b[4], p(logp), p(counts), p(visited), _lib.stream_ptr())

    for kw in (dict(batch=0), dict(n_ent=0), dict(n_ent=-5), dict(a=(keys, None, None, None, 4)), dict(b=(keys, None, None, None, 4)),
               dict(a=(None,) + _index_dev(c["index_a"]) + (len(c["index_a"][0]),))):            # an index without per-query keys
        assert call(**kw) != 0, kw
        assert b"rg_segment_eval" in L.rg_last_error(), kw
        torch.cuda.synchronize()
        assert (logp == -7.0).all() and (counts == -7).all() and (visited == -7).all(), kw    # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (counts != -7).all() and visited.tolist() == [1, 1, 0]
