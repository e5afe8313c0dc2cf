"""tests/rescore_ref.py against the CPU oracle (no GPU): re-scoring an answer on its r-digraph under a keep mask equals the oracle's
forward on the knowledge graph rebuilt without the masked facts.  float64, 1e-12 absolute (measured: a few 1e-16)."""
import numpy as np
import pytest

from tests import rescore_ref as R

TOL = 1e-12

_CACHE = {}


def _case(name):
    if name not in _CACHE:
        c = R.make_case(name, **R.CASES[name])
        c.keep = ~R.fact_mask(c.edges, c.n_rel, c.facts, c.fact_rows)
        c.res = R.rescore(c.params, c.edges, c.subs, c.rels, c.n_ent, c.L, c.act, keep=c.keep)
        c.orc = [R.oracle_without(c, b) for b in range(c.B)]
        _CACHE[name] = c
    return _CACHE[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_keep_none_reproduces_the_oracle(name):
    c = _case(name)
    score, reached, live, alpha = R.rescore(c.params, c.edges, c.subs, c.rels, c.n_ent, c.L, c.act)
    want = c.scores[np.arange(c.B), c.objs]
    print("%s: E %d, max |rescore - oracle| %.3g" % (name, len(c.edges), np.abs(score - want).max()))
    assert reached.all() and live.all() and (alpha > 0).all()
    assert np.abs(score - want).max() <= TOL


@pytest.mark.parametrize("name", list(R.CASES))
def test_deleted_facts_equal_the_rebuilt_graph(name):
    c = _case(name)
    score, reached, live, alpha = c.res
    want = np.array([o[0] for o in c.orc])
    member = np.array([o[1] for o in c.orc])
    print("%s: %d facts deleted, %d of %d edges kept, %d live; %d of %d rows reached; max |rescore - oracle| %.3g"
          % (name, len(c.facts), c.keep.sum(), len(c.edges), live.sum(), reached.sum(), c.B, np.abs(score - want).max()))
    # the condition on the inputs: both outcomes occur
    assert 4 * reached.sum() >= c.B and (~reached).any(), (name, int(reached.sum()), c.B)
    assert np.array_equal(reached, member)
    assert np.abs(score - want).max() <= TOL
    assert (score[~reached] == 0).all() and (want[~member] == 0).all()
    assert not live[~c.keep].any() and (alpha[~live] == 0).all() and (alpha[live] > 0).all()


@pytest.mark.parametrize("name", list(R.CASES))
def test_live_is_kept_and_head_visited_in_the_rebuilt_graph(name):
    """The forward sweep: a kept edge is live iff the oracle, on the graph without the row's facts, visits its head one hop down.
    Kept edges whose head is no longer visited (dangling) exist in every case and are reported dead."""
    c = _case(name)
    live = c.res[2]
    row, hop, head = c.edges[:, 0], c.edges[:, 1], c.edges[:, 2]
    visited = np.array([int(h) in c.orc[b][2][l - 1] for b, l, h in zip(row, hop, head)])
    assert np.array_equal(live, c.keep & visited)
    dangling = c.keep & ~visited
    print("%s: %d kept edges are dead" % (name, dangling.sum()))
    assert dangling.any() and not live[dangling].any()


def test_fp32_reference_is_close_to_fp64():
    c = _case("e300_L3")
    s64 = c.res[0]
    s32 = R.rescore(c.params, c.edges, c.subs, c.rels, c.n_ent, c.L, c.act, keep=c.keep, dtype=np.float32)[0]
    assert s32.dtype == np.float32 and np.abs(s32 - s64).max() < 1e-4
    assert np.array_equal(s32 == 0, s64 == 0)


def test_fact_mask_reference_on_a_typed_in_list():
    n_rel = 3
    edges = np.array([[0, 1, 5, 0, 6], [0, 1, 5, 6, 5], [0, 2, 6, 3, 5], [0, 2, 6, 6, 6], [1, 1, 5, 0, 6], [1, 2, 6, 3, 5], [1, 2, 5, 0, 6]])
    assert R.fact_mask(edges, n_rel, [(5, 0, 6)]).tolist() == [True, False, True, False, True, True, True]
    assert R.fact_mask(edges, n_rel, [(6, 3, 5)]).tolist() == [True, False, True, False, True, True, True]       # the twin names the same fact
    assert R.fact_mask(edges, n_rel, [(5, 0, 6)], rows=[1]).tolist() == [False, False, False, False, True, True, True]
    assert not R.fact_mask(edges, n_rel, [(5, 6, 5), (6, 6, 6)]).any()                                          # self-loops are no facts
    assert not R.fact_mask(edges, n_rel, np.zeros((0, 3), np.int64)).any()
