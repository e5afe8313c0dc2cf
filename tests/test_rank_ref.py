"""tests/rank_ref.py (the integer-counting form of rg_rank's formula that tests/test_rank_gpu.py compares the kernel with) checked on
the CPU against the oracle's cal_ranks - the reference's scipy.rankdata form - and against the fixture computed by the reference."""
import numpy as np
import pytest

from oracle import redgnn_oracle as orc
from tests import _util as U
from tests import rank_ref as rr


def test_rank_ref_by_hand():
    """scores [3, 1, 3, 0, 2]: min 0, s' = s + 1e-8.  Answer 4 (s = 2): entities 0 and 2 score higher, 0 is filtered (filter {0, 4}): 1 + (1 + 1) / 2 = 2.
    Answer 0 (s = 3): nothing higher, tied with entity 2: 0 + (2 + 1) / 2 = 1.5."""
    i32 = lambda *a: np.array(a, np.int32)
    got = rr.ranks(np.array([[3, 1, 3, 0, 2]], np.float32), i32(0, 2), i32(4, 0), i32(0, 2), i32(0, 4))
    assert got.tolist() == [2.0, 1.5]


def test_rank_ref_equals_the_fixture():
    fx = U.load("ranks.npz")
    csr = rr.to_csr(fx["labels"], fx["filters"])
    assert np.array_equal(rr.ranks(fx["scores"], *csr), fx["ranks"])


@pytest.mark.parametrize("n_ent", [1, 2, 255, 257, 1000])
def test_rank_ref_equals_cal_ranks(n_ent):
    """The batch the GPU test uses, on dense labels / filters through both of the oracle's forms.  Answers that repeat inside a list
    (n_ent < 50) collapse in the dense form, so the comparison goes through the dense form's own CSR."""
    scores, ap, ai, fp, fi = rr.batch(n_ent)
    labels, filters = rr.to_dense(n_ent, ap, ai, fp, fi)
    csr = rr.to_csr(labels, filters)
    want = rr.ranks(scores, *csr)
    assert np.array_equal(np.array(orc.cal_ranks(scores, labels, filters)), want)
    assert np.array_equal(np.array(orc.cal_ranks_closed_form(scores, labels, filters)), want)
    if n_ent >= 50:
        assert all(np.array_equal(a, b) for a, b in zip(csr, (ap, ai, fp, fi)))


def test_batch_holds_what_it_names():
    for n_ent in (1, 2, 255, 256, 257, 16368, 16369, 16384, 16385, 40000):
        scores, ap, ai, fp, fi = rr.batch(n_ent)
        assert np.isfinite(scores).all() and scores.dtype == np.float32 and ai.dtype == fi.dtype == np.int32
        n_ans, n_filt = np.diff(ap), np.diff(fp)
        assert n_ans[0] == 0 and n_filt[0] == 0 and n_ans[1] == 1 and (n_ans[2:] == 50).all()
        assert (n_filt[2:] >= min(n_ent, 300)).all() and (n_ent < 300 or n_filt.max() > 256)
        assert len(np.unique(scores[3])) == 1 and (scores[5] < 0).all()
        assert np.count_nonzero(scores[4]) == min(n_ent, 40) and (scores[4] >= 0).all()
        assert len(np.unique(scores[6])) <= min(n_ent, 100)
        for q in range(len(rr.ROW_KINDS)):      # a filter list is a set and holds the query's answers
            f, a = fi[fp[q]:fp[q + 1]], ai[ap[q]:ap[q + 1]]
            assert len(np.unique(f)) == len(f) and np.isin(a, f).all() and (len(f) == 0 or (0 <= f.min() and f.max() < n_ent))
        if n_ent >= 300:
            a4 = ai[ap[4]:ap[5]]
            assert (scores[4, a4] > 0).any() and (scores[4, a4] == 0).any()
