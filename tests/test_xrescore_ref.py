"""tests/xrescore_ref.py and tests/digraph_index_ref.py without a GPU: the reference rescore with every edge kept against
extrap_ref.walk's logits, the conditions of the inputs the GPU tests share (asserted with the reference alone), and the numpy statement
of the per-hop index against hand-written expectations."""
import functools
import re

import numpy as np
import pytest

from tests import digraph_index_ref as IR
from tests import extrap_ref as XR
from tests import xrescore_ref as R
from tests.test_extrap_ref import _state

CASES = XR.CASES + [(32, 30, "relu", 4, 5)]


@functools.lru_cache(maxsize=None)
def _case(d, a, act, L, B):
    from oracle import redgnn_oracle as orc
    data, q = XR.make_case(d, B)
    q = R.queries_of_case(data, q)
    off = orc.get_time_offset_list(data, 24)
    p = _state(d, a, L)
    logits, last, hops, cur_t = XR.walk(p, data, off, 24, XR.N_ENT, XR.N_REL, q[:, 0], q[:, 1], q[:, 3], L, act)
    q_of, objs = R.rows_of_case(q, hops, last, data)
    edges, data_row, day, reached = R.digraph_of(hops, q_of, objs, last, XR.N_ENT)
    return data, q, p, logits, last, cur_t, q_of, objs, edges, data_row, day, reached


@pytest.mark.parametrize("d,a,act,L,B", CASES)
def test_every_edge_kept_is_the_walk(d, a, act, L, B):
    data, q, p, logits, last, cur_t, q_of, objs, edges, data_row, day, reached = _case(d, a, act, L, B)
    score, got_reached, live, alpha = R.rescore(p, edges, day, cur_t[q_of], q[q_of, 0], q[q_of, 1], XR.N_ENT, L, act)
    assert np.array_equal(got_reached, reached) and reached.any() and not reached.all() and live.all()
    key = last[:, 0] * XR.N_ENT + last[:, 1]
    want = logits[np.searchsorted(key, (q_of * XR.N_ENT + objs)[reached])]
    np.testing.assert_allclose(score[reached], want, rtol=1e-10, atol=0)
    assert (score[~reached] == 0).all() and ((alpha >= 0) & (alpha <= 1)).all()
    # the digraph's own structure: ordered by (row, hop, tail), self-loops carry no data row, data rows are the data's
    assert np.array_equal(edges[np.lexsort((edges[:, 4], edges[:, 1], edges[:, 0]))][:, [0, 1, 4]], edges[:, [0, 1, 4]])
    loop = data_row < 0
    assert (edges[loop, 3] == XR.N_REL).all() and np.array_equal(data[data_row[~loop], :3], edges[~loop][:, 2:5])
    assert np.array_equal(day[~loop], data[data_row[~loop], 3] // 24)


@pytest.mark.parametrize("d,a,act,L,B", CASES)
def test_the_shared_inputs_meet_their_conditions(d, a, act, L, B):
    data, q, p, logits, last, cur_t, q_of, objs, edges, data_row, day, reached = _case(d, a, act, L, B)
    heads, rels, q_day = q[q_of, 0], q[q_of, 1], cur_t[q_of]
    facts = R.deleted_facts(data, edges, data_row, day, heads)
    gone = R.rows_of_facts(data, facts)
    day_of = data[:, 3] // 24
    last_of_day = np.nonzero(np.append(day_of[1:] != day_of[:-1], True))[0]
    assert len(facts) >= 2 and not np.isin(gone, last_of_day).any(), "a deleted data row is the last row of its day"
    assert np.array_equal(np.unique(day_of), np.unique(R.without_rows(data, gone)[:, 3] // 24)), "a day loses all its rows"
    assert {9, 10, 11, 12, 13} <= set(gone.tolist())                      # one of the equal rows is listed: all five copies go
    m = R.fact_mask(edges, day, data_row, XR.N_REL, facts)
    assert np.array_equal(m, R.data_row_mask(edges, data_row, gone)), "the facts' rows and the rows' facts mark other edges"
    dup = np.isin(data_row, np.arange(9, 14))
    assert dup.sum() >= 5 and m[dup].all() and sorted(set(data_row[dup].tolist())) == [9, 10, 11, 12, 13]
    assert not m[data_row < 0].any()
    keep = ~m
    full = R.rescore(p, edges, day, q_day, heads, rels, XR.N_ENT, L, act)
    cut = R.rescore(p, edges, day, q_day, heads, rels, XR.N_ENT, L, act, keep=keep)
    n = len(q_of)
    print("d%d L%d: %d facts (%d data rows) deleted, %d of %d edges kept, %d live, %d of %d rows reached (%d before)"
          % (d, L, len(facts), len(gone), keep.sum(), len(edges), cut[2].sum(), cut[1].sum(), n, full[1].sum()))
    assert 4 * cut[1].sum() >= n and (full[1] & ~cut[1]).any(), "a quarter of the rows must stay reached and one be cut off"
    assert (keep & ~cut[2]).any(), "some kept edge must dangle"
    assert (cut[0][~cut[1]] == 0).all() and (cut[3][~cut[2]] == 0).all()
    # a hub: a destination of hop >= 2 with more than CHUNK live edges, before and after
    for live in (full[2], cut[2]):
        at = np.nonzero(live & (edges[:, 1] >= 2))[0]
        _, counts = np.unique(np.stack([edges[at, 0], edges[at, 1], edges[at, 4]], 1), axis=0, return_counts=True)
        assert counts.max() > R.CHUNK, "no destination with more than %d live edges (%d)" % (R.CHUNK, counts.max())
    # the twin of a fact: with the relations read as r / r + 3 the mask grows or stays
    assert (R.fact_mask(edges, day, data_row, XR.N_REL, facts, inverse_offset=3) >= m).all()
    assert not R.fact_mask(edges, day, data_row, XR.N_REL, np.zeros((0, 4), np.int64)).any()


# ---- the per-hop index on a hand-made digraph: 2 rows, 2 hops, n_ent = 10 -------------------------------------------------------------
EDGES = np.array([[0, 1, 3, 0, 3], [0, 1, 3, 1, 4], [0, 1, 3, 2, 4], [0, 2, 3, 0, 7], [0, 2, 4, 1, 7], [0, 2, 5, 1, 7],
                  [1, 1, 6, 0, 4], [1, 2, 4, 2, 4], [1, 2, 4, 0, 4]])
OFFSETS = np.array([0, 6, 9])
TIME = np.arange(9) + 20


def test_hop_index_reference_by_hand():
    assert IR.hop_ranges(EDGES, OFFSETS, 2).tolist() == [[0, 3, 6], [6, 7, 9]]
    keys0 = np.array([3, 16])
    h1 = IR.hop_index(EDGES, OFFSETS, 1, 2, keys0, 10, 3, edge_time=TIME)
    assert h1["at"].tolist() == [0, 1, 2, 6] and h1["src"].tolist() == [0, 0, 0, 1] and h1["rel"].tolist() == [0, 1, 2, 0]
    assert h1["time"].tolist() == [20, 21, 22, 26] and h1["keys"].tolist() == [3, 4, 14] and h1["dst_ptr"].tolist() == [0, 1, 3, 4]
    assert h1["row_of"].tolist() == [0, 0, 1] and h1["prev_idx"].tolist() == [0, -1, -1]
    h2 = IR.hop_index(EDGES, OFFSETS, 2, 2, h1["keys"], 10, 3)
    assert h2["at"].tolist() == [3, 4, 7, 8] and h2["src"].tolist() == [0, 1, 2, 2]          # edge 5's head 5 was never visited
    assert h2["keys"].tolist() == [7, 14] and h2["dst_ptr"].tolist() == [0, 2, 4] and h2["prev_idx"].tolist() == [-1, 2] and h2["time"] is None
    keep = np.array([1, 0, 0, 1, 1, 1, 1, 1, 0], bool)
    k1 = IR.hop_index(EDGES, OFFSETS, 1, 2, keys0, 10, 3, keep=keep)
    assert k1["at"].tolist() == [0, 6] and k1["keys"].tolist() == [3, 14] and k1["dst_ptr"].tolist() == [0, 1, 2]
    k2 = IR.hop_index(EDGES, OFFSETS, 2, 2, k1["keys"], 10, 3, keep=keep)
    assert k2["at"].tolist() == [3, 7] and k2["src"].tolist() == [0, 1]                      # edge 4 is kept and dangles
    none = IR.hop_index(EDGES, OFFSETS, 1, 2, keys0, 10, 3, keep=np.zeros(9, bool))
    assert len(none["at"]) == len(none["keys"]) == len(none["dst_ptr"]) == 0
    for col, row, value, text in ((4, 2, 2, IR.ORDER), (4, 5, 8, None), (4, 3, 6, IR.TWO_TAILS), (2, 0, 10, IR.ENTITY), (3, 1, 3, IR.RELATION), (0, 6, 0, IR.ROW_HOP),
                                  (1, 1, 2, IR.ROW_HOP)):
        bad = EDGES.copy()
        bad[row, col] = value
        run = lambda: [IR.hop_index(bad, OFFSETS, l, 2, keys0 if l == 1 else h1["keys"], 10, 3) for l in (1, 2)]
        if text is None:                                 # a second tail on an edge that is not live is no second node
            assert run()[1]["keys"].tolist() == [7, 14]
            continue
        with pytest.raises(ValueError, match=re.escape(text)):
            run()
