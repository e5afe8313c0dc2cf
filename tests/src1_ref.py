"""The test graph of the single-source walk (rg_layer_fwd walk 8) and a numpy statement of the out-list it reads.  TEST INFRASTRUCTURE.

The out-list is a second CSR-by-head over the library's out_ptr in which every head's out-edges are ordered by (tail, position of the
edge in the CSR-by-tail); the CSR-by-tail keeps fact-row order inside a tail (include/redgnn.h rg_graph_create), and the fact rows are
the triples, their inverses, then one identity row per entity (load_data.py:69-80 of the reference)."""
import numpy as np

N_ENT, N_REL = 300, 3
HUB, ISOLATED, MULTI_HEAD, MULTI_TAIL, SPAN_HEAD = 0, N_ENT - 1, 10, 11, 12


def make_triples(seed=5):
    """About 3000 triples over entities 0 .. 298 (299 keeps only its self-loop).  Entity 0 is a hub: head of 320 triples and tail of 200
    (so in- and out-degree of the doubled graph pass 500: its CSR rows are cut into 128-entry segments and its out-list needs several
    chunks).  (10, r, 11) holds for all three relations, in relation order 2, 0, 1 (fact order, not relation order, must decide).
    (12, r, 0) holds for three relations at the start, the middle and the end of the triple list: three edges 12 -> hub whose CSR-by-tail
    positions lie in different segments of the hub's row."""
    rng = np.random.default_rng(seed)
    m = 2400
    top = N_ENT - 1
    h, t = rng.integers(1, top, m), rng.integers(1, top, m)
    trip = np.stack([h, rng.integers(0, N_REL, m), t], 1)
    hub_out = np.stack([np.full(320, HUB), rng.integers(0, N_REL, 320), rng.integers(1, top, 320)], 1)
    hub_in = np.stack([rng.integers(1, top, 200), rng.integers(0, N_REL, 200), np.full(200, HUB)], 1)
    body = np.concatenate([trip, hub_out, hub_in], 0)
    body = body[rng.permutation(len(body))]
    multi = np.array([[MULTI_HEAD, 2, MULTI_TAIL], [MULTI_HEAD, 0, MULTI_TAIL], [MULTI_HEAD, 1, MULTI_TAIL]])
    k = len(body) // 2
    return np.concatenate([[[SPAN_HEAD, 1, HUB]], body[:k], [[SPAN_HEAD, 0, HUB]], multi, body[k:], [[SPAN_HEAD, 2, HUB]]], 0).astype(np.int64)


def subjects(seed=6, B=33):
    """33 queries: the hub, the isolated entity, the multi-edge heads, one subject twice (with two relations), the rest random."""
    rng = np.random.default_rng(seed)
    sub = rng.integers(0, N_ENT, B)
    rel = rng.integers(0, 2 * N_REL, B)
    sub[:6] = (HUB, ISOLATED, MULTI_HEAD, SPAN_HEAD, 77, 77)
    rel[4:6] = (0, 4)
    return sub.astype(np.int64), rel.astype(np.int64)


def fact_rows(triples, n_ent=N_ENT, n_rel=N_REL):
    """(H, R, T) of the library's fact rows: triples, inverses (rel + n_rel), identity (rel 2 n_rel)."""
    tr = np.asarray(triples, np.int64)
    ent = np.arange(n_ent)
    H = np.concatenate([tr[:, 0], tr[:, 2], ent])
    R = np.concatenate([tr[:, 1], tr[:, 1] + n_rel, np.full(n_ent, 2 * n_rel)])
    T = np.concatenate([tr[:, 2], tr[:, 0], ent])
    return H, R, T


def out_by_tail(triples, n_ent=N_ENT, n_rel=N_REL):
    """(out_ptr, rel_tail [n_fact, 2], pos [n_fact], in_ptr, in_head_rel [n_fact, 2]) as the library must build them."""
    H, R, T = fact_rows(triples, n_ent, n_rel)
    by_tail = np.argsort(T, kind="stable")                       # CSR-by-tail: fact order inside a tail
    in_ptr = np.concatenate([[0], np.cumsum(np.bincount(T, minlength=n_ent))])
    in_hr = np.stack([H[by_tail], R[by_tail]], 1)
    pos_of_fact = np.empty(len(H), np.int64)
    pos_of_fact[by_tail] = np.arange(len(H))
    order = np.lexsort((pos_of_fact, T, H))                      # by head, then tail, then CSR-by-tail position
    out_ptr = np.concatenate([[0], np.cumsum(np.bincount(H, minlength=n_ent))])
    return out_ptr, np.stack([R[order], T[order]], 1), pos_of_fact[order], in_ptr, in_hr


def check_out_by_tail(out_ptr, rel_tail, pos, in_ptr, in_hr):
    """The properties the walk relies on, from the arrays alone: pos is a permutation of the CSR-by-tail, entry j of head h's row is the
    CSR-by-tail entry pos[j] (same head, relation, tail), and inside a row (tail, pos) increases strictly."""
    out_ptr, rel_tail, pos, in_ptr, in_hr = (np.asarray(x, np.int64) for x in (out_ptr, rel_tail, pos, in_ptr, in_hr))
    n_fact, n_ent = len(pos), len(out_ptr) - 1
    assert out_ptr[0] == 0 and out_ptr[-1] == n_fact and in_ptr[-1] == n_fact
    assert np.array_equal(np.sort(pos), np.arange(n_fact))
    head = np.repeat(np.arange(n_ent), np.diff(out_ptr))
    tail_of_pos = np.repeat(np.arange(n_ent), np.diff(in_ptr))
    assert np.array_equal(in_hr[pos, 0], head) and np.array_equal(in_hr[pos, 1], rel_tail[:, 0])
    assert np.array_equal(tail_of_pos[pos], rel_tail[:, 1])
    key = rel_tail[:, 1] * n_fact + pos                          # (tail, pos) as one number
    same_row = head[1:] == head[:-1]
    assert (np.diff(key)[same_row] > 0).all()
