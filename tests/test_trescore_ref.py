"""tests/trescore_ref.py against the float64 walk of tests/temporal_ref.py (no GPU): re-scoring an answer on its temporal r-digraph
under a keep mask equals the walk on the quadruple graph rebuilt without the masked quadruples (and their inverse twins).  float64,
1e-12 absolute (measured: a few 1e-16).  The inputs of the GPU tests (tests/test_trescore_gpu.py) are chosen here and their
conditions asserted with the reference alone."""
import numpy as np
import pytest

from tests import temporal_ref as TR
from tests import trescore_ref as R
from tests.test_temporal_ref import random_params

TOL = 1e-12
N_ENT, N_ROWS_TAB, N_TIME = TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1, TR.HAND_N_TIME
CASES = [(2, False, "relu"), (3, False, "tanh"), (2, True, "idd"), (3, True, "relu")]      # (L, shared tables, act)

_CACHE = {}


def _case(L, shared, act):
    key = (L, shared, act)
    if key not in _CACHE:
        quads, heads, rels, times, objs, deleted = R.inputs(L)
        p = random_params(np.random.default_rng(10 * L + shared), N_ROWS_TAB, N_TIME, L, 20, 5, shared)
        edges, etime, reached = R.digraph_of(quads, heads, objs, L)
        full = TR.walk(p, quads, N_ENT, heads, rels, times, L, act, shared_tables=shared)
        cut_quads = R.without_quads(quads, deleted, R.INVERSE_OFFSET)
        cut = TR.walk(p, cut_quads, N_ENT, heads, rels, times, L, act, shared_tables=shared)
        mask = R.fact_mask(edges, etime, R.IDENTITY, deleted, inverse_offset=R.INVERSE_OFFSET)
        res = R.rescore(p, edges, etime, heads, rels, times, N_ENT, L, act, keep=~mask, shared_tables=shared)
        _CACHE[key] = dict(quads=quads, heads=heads, rels=rels, times=times, objs=objs, deleted=deleted, p=p, edges=edges, etime=etime,
                           reached=reached, full=full, cut=cut, cut_quads=cut_quads, mask=mask, res=res)
    return _CACHE[key]


def test_the_queries_cover_what_the_issue_names():
    quads, heads, rels, times, objs, deleted = R.inputs(2)
    assert {2, 3, 299} <= set(heads.tolist()) and any(256 <= h <= 298 for h in heads.tolist())
    assert set(times.tolist()) == {0, 2, 8, 11}
    assert (3, 0, 0, 2) in set(map(tuple, deleted.tolist())) and (3, 0, 0, 8) not in set(map(tuple, deleted.tolist()))
    assert (np.all(quads == (3, 0, 0, 2), 1)).sum() == 2                      # the exact duplicate
    for L in (2, 3):
        edges, etime, reached = R.digraph_of(quads, heads, objs, L)
        assert reached.all()
        for l in range(2, L + 1):                                             # hub 2: a destination of 129 in-edges from hop 2 on
            hub = (edges[:, 0] == 0) & (edges[:, 1] == l) & (edges[:, 4] == 2)
            assert hub.sum() == 129
            dirs = TR.direction(etime[hub], times[0])
            assert set(dirs.tolist()) == {1, 2}                               # query time 0: now and future
        hub = (edges[:, 0] == 8) & (edges[:, 1] == 2) & (edges[:, 4] == 2)    # query time 8: past, now and future on one destination
        assert hub.sum() == 129 and set(TR.direction(etime[hub], times[8]).tolist()) == {0, 1, 2}


@pytest.mark.parametrize("L,shared,act", CASES)
def test_keep_none_reproduces_the_walk(L, shared, act):
    c = _case(L, shared, act)
    score, reached, live, alpha = R.rescore(c["p"], c["edges"], c["etime"], c["heads"], c["rels"], c["times"], N_ENT, L, act,
                                            shared_tables=shared)
    want = c["full"][0][np.arange(len(c["objs"])), c["objs"]]
    print("L%d shared=%s: E %d, max |rescore - walk| %.3g" % (L, shared, len(c["edges"]), np.abs(score - want).max()))
    assert reached.all() and live.all() and (alpha > 0).all()
    assert np.abs(score - want).max() <= TOL


@pytest.mark.parametrize("L,shared,act", CASES)
def test_deleted_quadruples_equal_the_rebuilt_graph(L, shared, act):
    c = _case(L, shared, act)
    score, reached, live, alpha = c["res"]
    B = len(c["objs"])
    scores, _, last = c["cut"]
    want = scores[np.arange(B), c["objs"]]
    member = np.array([(b, int(o)) in set(map(tuple, last.tolist())) for b, o in enumerate(c["objs"])])
    keep = ~c["mask"]
    print("L%d shared=%s: %d quadruples deleted, %d of %d edges kept, %d live; %d of %d rows reached; max |rescore - walk| %.3g"
          % (L, shared, len(c["deleted"]), keep.sum(), len(keep), live.sum(), reached.sum(), B, np.abs(score - want).max()))
    assert len(c["cut_quads"]) == len(c["quads"]) - 2 * len(c["deleted"]) - 2      # each with its twin; (3, 0, 0, 2) twice
    # the conditions on the inputs: a quarter of the rows stay reached, one is cut off, a kept edge dangles
    assert 4 * reached.sum() >= B and (~reached).any(), (int(reached.sum()), B)
    assert (keep & ~live).any()
    assert np.array_equal(reached, member)
    assert np.abs(score - want).max() <= TOL
    assert (score[~reached] == 0).all() and (want[~member] == 0).all()
    assert not live[~keep].any() and (alpha[~live] == 0).all() and (alpha[live] > 0).all()


@pytest.mark.parametrize("L", [2, 3])
def test_live_is_kept_and_head_visited_in_the_rebuilt_graph(L):
    c = _case(L, False, "relu" if L == 2 else "tanh")
    live, keep = c["res"][2], ~c["mask"]
    levels = R.level_sets(c["cut_quads"], c["heads"], L)
    visited = np.array([int(h) in levels[b][l - 1] for b, l, h in c["edges"][:, :3].tolist()])
    assert np.array_equal(live, keep & visited)


def test_both_copies_of_the_duplicate_go_and_the_other_time_stays():
    c = _case(2, False, "relu")
    e, t = c["edges"], c["etime"]
    fact = (e[:, 2] == 3) & (e[:, 3] == 0) & (e[:, 4] == 0) & (e[:, 0] == 1) & (e[:, 1] == 1)         # row 1 = (3, ., time 2) -> 0, hop 1
    assert sorted(t[fact].tolist()) == [2, 2, 8]
    assert c["mask"][fact & (t == 2)].all() and not c["mask"][fact & (t == 8)].any()
    twin = (e[:, 2] == 0) & (e[:, 3] == 3) & (e[:, 4] == 3) & (e[:, 0] == 15)                        # row 15 = (0, ., .) -> 3: the inverse
    assert (twin & (t == 2)).sum() == 4 and (twin & (t == 8)).sum() == 2 and c["mask"][twin & (t == 2)].all()    # at hop 1 and at hop 2
    assert not c["mask"][twin & (t == 8)].any()
    assert c["res"][1][[1, 10, 15]].all()                                    # still reached, through the time-8 quadruple
    only = R.fact_mask(e, t, R.IDENTITY, [(3, 0, 0, 2)])                     # no twins: the inverse edges stay
    assert only[fact & (t == 2)].all() and not only[twin].any()


def test_fp32_reference_is_close_to_fp64():
    c = _case(3, False, "tanh")
    s64 = c["res"][0]
    s32 = R.rescore(c["p"], c["edges"], c["etime"], c["heads"], c["rels"], c["times"], N_ENT, 3, "tanh", keep=~c["mask"], dtype=np.float32)[0]
    assert s32.dtype == np.float32 and np.abs(s32 - s64).max() < 1e-4
    assert np.array_equal(s32 == 0, s64 == 0)


def test_fact_mask_reference_on_a_typed_in_list():
    edges = np.array([[0, 1, 5, 0, 6], [0, 1, 5, 0, 6], [0, 1, 5, 6, 5], [0, 2, 6, 3, 5], [0, 2, 6, 6, 6], [1, 1, 5, 0, 6], [1, 2, 6, 3, 5]])
    time = np.array([2, 4, 11, 2, 11, 2, 4])
    f = lambda facts, **kw: R.fact_mask(edges, time, 6, facts, **kw).tolist()
    assert f([(5, 0, 6, 2)]) == [True, False, False, False, False, True, False]
    assert f([(5, 0, 6, 2)], inverse_offset=3) == [True, False, False, True, False, True, False]
    assert f([(6, 3, 5, 2)], inverse_offset=3) == [True, False, False, True, False, True, False]      # the twin names the same fact
    assert f([(5, 0, 6, 4)], rows=[1], inverse_offset=3) == [False] * 6 + [True]
    assert not any(f([(5, 6, 5, 11), (6, 6, 6, 11)], inverse_offset=3))                               # the identity is no fact
    assert not any(f(np.zeros((0, 4), np.int64)))
