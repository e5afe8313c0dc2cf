"""tests/trule_ground_ref.py against itself and against paper (no GPU): the definition (counts_dense) and the edge-list form (counts)
agree on the hand graph and on a random graph, the hand graph's counts are the ones written next to it, and with a single time id and
every step "any" a temporal rule is the static rule on the time-stripped rows."""
import numpy as np

from tests import rule_ground_ref as R
from tests import trule_ground_ref as T


def _invariants(c):
    assert (c >= 0).all()
    assert (c[:, 1] <= c[:, 2]).all() and (c[:, 2] <= c[:, 0]).all() and (c[:, 1] <= c[:, 3]).all()


def _hand():
    return T.HAND_N_ENT, T.HAND_N_RELA, T.HAND_N_TIME, T.hand_quads()


def test_hand_counts():
    n_ent, n_rela, n_time, quads = _hand()
    assert np.array_equal(T.default_anchors(quads, n_ent, n_rela), T.HAND_ANCHORS)
    for f in (T.counts_dense, T.counts):
        assert np.array_equal(f(n_ent, n_rela, n_time, quads, T.HAND_HEAD, T.HAND_BODY, T.HAND_DIR), T.HAND_ALL), f.__name__
        assert np.array_equal(f(n_ent, n_rela, n_time, quads, T.HAND_HEAD, T.HAND_BODY, T.HAND_DIR, T.HAND_SUBSET), T.HAND_SUB), f.__name__
        assert np.array_equal(f(n_ent, n_rela, n_time, quads, T.HAND_HEAD, T.HAND_BODY, T.HAND_DIR, T.HAND_SUBSET[::-1]), T.HAND_SUB)
    _invariants(T.HAND_ALL)
    _invariants(T.HAND_SUB)
    # the steps of the hand rules cover the four directions, an identity step and an empty relation
    assert set(T.HAND_DIR.reshape(-1).tolist()) == {0, 1, 2, 3} and (T.HAND_BODY == T.HAND_N_RELA - 1).any()
    assert not (quads[:, 1] == 2).any() and (T.HAND_BODY == 2).any()
    # the fact at two times and the exact duplicate are in the rows
    assert len(quads) > len(np.unique(quads, axis=0)) and len(np.unique(quads[:, :3], axis=0)) < len(np.unique(quads, axis=0))


def test_counts_sum_over_disjoint_anchor_sets():
    n_ent, n_rela, n_time, quads = _hand()
    parts = [T.counts(n_ent, n_rela, n_time, quads, T.HAND_HEAD, T.HAND_BODY, T.HAND_DIR, T.HAND_ANCHORS[lo:hi])
             for lo, hi in ((0, 3), (3, 4), (4, 10))]
    assert np.array_equal(sum(parts), T.HAND_ALL)


def _random_graph(seed=3, n_ent=30, n_rel=3, n_time=5, m=150):
    rng = np.random.default_rng(seed)
    base = np.column_stack([rng.integers(0, n_ent, m), rng.integers(0, n_rel, m), rng.integers(0, n_ent, m), rng.integers(0, n_time, m)])
    base = np.concatenate([base, base[:10]], 0)                                   # ten exact duplicates
    base = np.concatenate([base, np.column_stack([base[:10, :3], (base[:10, 3] + 1) % n_time])], 0)      # ten facts at a second time
    ent = np.arange(n_ent)
    quads = np.concatenate([base, np.column_stack([base[:, 2], base[:, 1] + n_rel, base[:, 0], base[:, 3]]),
                            np.column_stack([ent, np.full(n_ent, 2 * n_rel), ent, np.full(n_ent, n_time - 1)])], 0)
    return n_ent, 2 * n_rel + 1, n_time, quads, rng


def test_dense_and_edge_list_forms_agree_on_a_random_graph():
    n_ent, n_rela, n_time, quads, rng = _random_graph()
    every = np.stack(np.meshgrid(np.arange(n_ent), np.arange(n_time), indexing="ij"), -1).reshape(-1, 2)      # 150 anchors: 3 words of 64
    some_body = some_hits = 0
    for L, (head, body, direc) in T.random_rules(rng, 45, n_rela).items():
        for anchors in (None, every, every[rng.permutation(len(every))[:33]]):
            a = T.counts_dense(n_ent, n_rela, n_time, quads, head, body, direc, anchors)
            b = T.counts(n_ent, n_rela, n_time, quads, head, body, direc, anchors)
            assert np.array_equal(a, b), L
            _invariants(a)
            some_body += int((a[:, 0] > 0).sum())
            some_hits += int((a[:, 1] > 0).sum())
    assert some_body > 5 and some_hits > 0                                         # the comparison is not one of zeros


def test_single_time_and_any_steps_are_the_static_rule():
    n_ent, n_rela, _, quads, rng = _random_graph(seed=4)
    quads = quads.copy()
    quads[:, 3] = 0
    head, body = rng.integers(0, n_rela, 30), rng.integers(0, n_rela, (30, 2))
    every = np.column_stack([np.arange(n_ent), np.zeros(n_ent, np.int64)])
    t = T.counts(n_ent, n_rela, 1, quads, head, body, np.full_like(body, T.ANY), every)
    s = R.counts(n_ent, n_rela, quads[:, :3], head, body)
    assert np.array_equal(t[:, 0], s[:, 0]) and (t[:, 0] > 0).any()
    # with one time id "now" is "any" too, and the head step is then the static head: all four counts agree
    assert np.array_equal(T.counts(n_ent, n_rela, 1, quads, head, body, np.full_like(body, T.NOW), every), s)
    assert np.array_equal(t, s)
