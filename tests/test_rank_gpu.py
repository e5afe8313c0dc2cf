"""rg_rank called on its own, through engine.rank on CSR lists, against the integer-counting reference of tests/rank_ref.py: exact
equality, no tolerance.  n_ent runs over both sides of the kernel's staging boundary: the LDS-staged kernel takes rows whose
n_ent * 4 bytes plus the kernel's 64 bytes of static LDS fit the 64 KiB a launch may request, n_ent <= 16368 (rank.hip, rg_rank);
before, the condition was n_ent <= 16384, whose last 16 sizes asked for more than that.  Each batch (rank_ref.batch) holds a query
without answers and with an empty filter list, one with a single answer, 50 answers inside a filter list of 300 entries, a row of
equal scores, a row of zeros with a few positives, a row of negatives and a row of heavy ties.
"""
import numpy as np
import pytest
import torch

from tests import rank_ref as rr

pytestmark = pytest.mark.gpu

N_ENT = [1, 2, 255, 256, 257, 16368, 16369, 16384, 16385, 40000]


def _rank(scores, csr):
    from red_gnn_amd import engine as eng
    dev = [torch.as_tensor(a).cuda() for a in csr]
    if dev[1].numel() == 0 or dev[3].numel() == 0:      # engine.rank passes data pointers: keep them non-NULL
        raise AssertionError("empty lists")
    out = eng.rank(torch.as_tensor(scores).cuda(), *dev)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("n_ent", N_ENT)
def test_rank_equals_reference(n_ent):
    scores, *csr = rr.batch(n_ent)
    want = rr.ranks(scores, *csr)
    got = _rank(scores, csr)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "n_ent %d: %d of %d ranks differ; first at answer %d: gpu %s ref %s" % (n_ent, bad.size, want.size, bad[0],
                                                                                                   got[bad[0]], want[bad[0]])
    assert np.array_equal(_rank(scores, csr), got), "n_ent %d: second run differs" % n_ent
    print("n_ent %d: %d ranks, min %.1f max %.1f" % (n_ent, want.size, want.min(), want.max()))


def test_rank_of_the_fixture_through_csr():
    """The reference's own ranks (tests/golden/ranks.npz), from CSR lists."""
    from tests import _util as U
    fx = U.load("ranks.npz")
    csr = rr.to_csr(fx["labels"], fx["filters"])
    assert np.array_equal(_rank(fx["scores"].astype(np.float32), csr), fx["ranks"])
