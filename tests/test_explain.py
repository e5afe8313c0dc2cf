"""CPU checks of the r-digraph extraction (-m "not gpu"): the C-ABI's argument errors, no silent CPU path, and
RDigraph.strongest_paths against a brute-force enumeration of the paths of hand-built digraphs."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import _util as U


def test_explain_entry_points_report_bad_arguments():
    from red_gnn_amd import _lib
    L = _lib.lib()
    buf = np.zeros(64, np.int32)
    p = _lib.ptr(buf)
    n_e = C.c_int64()
    assert L.rg_explain_scratch_bytes(None) == 0
    # a NULL frontier
    assert L.rg_explain_seed(None, 4, 10, 1, p, p, p, None) != 0
    assert b"NULL frontier" in L.rg_last_error()
    assert L.rg_explain_count(None, None, 4, 10, 1, p, p, p, p, 4, p, p, 3, 0.0, p, p, p, 256, C.byref(n_e), None) != 0
    assert b"NULL frontier" in L.rg_last_error()
    assert L.rg_explain_emit(None, None, 4, 10, 1, p, p, p, p, 4, p, p, 3, 0.0, p, p, p, None) != 0
    assert b"NULL frontier" in L.rg_last_error()
    # a hop level out of range (before anything else is looked at)
    for level in (0, -1, 16):
        assert L.rg_explain_count(None, None, 4, 10, level, p, p, p, p, 4, p, p, 3, 0.0, p, p, p, 256, C.byref(n_e), None) != 0
        assert b"level" in L.rg_last_error()
        assert L.rg_explain_seed(None, 4, 10, level, p, p, p, None) != 0
        assert b"level" in L.rg_last_error()
    # a batch / entity count that cannot match any frontier
    assert L.rg_explain_emit(None, None, 0, 10, 1, p, p, p, p, 4, p, p, 3, 0.0, p, p, p, None) != 0
    assert b"batch=0" in L.rg_last_error()
    assert L.rg_explain_seed(None, 4, -3, 1, p, p, p, None) != 0
    assert b"n_ent=-3" in L.rg_last_error()
    assert L.rg_explain_gather(-1, 1, 4, p, p, p, p, 0, p, p, None) != 0
    assert b"rg_explain_gather" in L.rg_last_error()
    assert L.rg_explain_gather(0, 1, 4, None, None, None, None, 0, None, None, None) == 0      # nothing to do


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_explain_fails_loudly_without_gpu():
    from red_gnn_amd import _lib
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    ids = U.load("tiny_fwd.npz")
    loader = DataLoader(ids=ids, verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 2, 16, 3, loader.n_rel, "relu", 0.0

    model = RED_GNN_trans(P, loader)
    with pytest.raises(_lib.NativeError):
        model.explain(ids["subs"], ids["rels"], np.zeros(len(ids["subs"]), np.int64))
    with pytest.raises(_lib.NativeError):
        model.explain(ids["subs"], ids["rels"])


def _digraph(rows, L):
    """RDigraph from per-row lists of (hop, head, rel, tail, alpha), in the stated order (the CSR position is taken as (head, rel))."""
    from red_gnn_amd.explain import RDigraph
    e, a, off = [], [], [0]
    for b, lst in enumerate(rows):
        lst = sorted(lst, key=lambda x: (x[0], x[3], x[1], x[2]))
        e += [(b, h, hd, r, t) for (h, hd, r, t, _) in lst]
        a += [al for (*_, al) in lst]
        off.append(len(e))
    B = len(rows)
    return RDigraph(edges=torch.tensor(e, dtype=torch.int32).reshape(-1, 5), alpha=torch.tensor(a, dtype=torch.float32),
                    offsets=torch.tensor(off, dtype=torch.int64), reached=torch.tensor([len(r) > 0 for r in rows]),
                    score=torch.zeros(B), n_hops=L)


def _brute(lst, L, s):
    """All length-L paths from s through the hop-labelled edges; best product (float64, left to right), ties: the smallest
    (head, rel) at the last step, then the one before, ..."""
    by_hop = {l: [x for x in lst if x[0] == l] for l in range(1, L + 1)}
    best = None
    for combo in itertools.product(*[by_hop[l] for l in range(1, L + 1)]):
        if combo[0][1] != s or any(combo[k][3] != combo[k + 1][1] for k in range(L - 1)):
            continue
        prod = 1.0
        for x in combo:
            prod = prod * float(np.float32(x[4]))
        key = (-prod,) + tuple(v for x in reversed(combo) for v in (x[1], x[2]))
        if best is None or key < best[0]:
            best = (key, combo, prod)
    if best is None:
        return [-1] * L, [-1] * (L + 1), 0.0
    combo = best[1]
    return [x[2] for x in combo], [combo[0][1]] + [x[3] for x in combo], best[2]


def _random_rows(rng, B, L, n_ent, n_rel, vals):
    rows, starts = [], []
    for b in range(B):
        s = int(rng.integers(n_ent))
        o = int(rng.integers(n_ent))
        starts.append(s)
        if b % 5 == 4:
            rows.append([])                           # an unreached row
            continue
        levels = [[s]] + [sorted(set(rng.integers(0, n_ent, rng.integers(1, 4)).tolist())) for _ in range(L - 1)] + [[o]]
        lst = []
        for l in range(1, L + 1):
            for t in levels[l]:
                for h in levels[l - 1]:
                    for r in set(rng.integers(0, n_rel, rng.integers(1, 3)).tolist()):
                        lst.append((l, h, r, t, float(rng.choice(vals))))
        # keep only edges on an s -> o path (every node of a level has an in- and out-edge here, so all are)
        rows.append(lst)
    return rows, starts


@pytest.mark.parametrize("L", [1, 2, 3, 4])
def test_strongest_paths_match_brute_force(L):
    rng = np.random.default_rng(L)
    vals = [0.5, 0.25, 0.75, 1.0, 0.125]                 # few significant bits: products exact in float64, ties frequent
    rows, starts = _random_rows(rng, 12, L, 6, 3, vals)
    rd = _digraph(rows, L)
    rl, en, pr = rd.strongest_paths()
    for b, lst in enumerate(rows):
        r_ref, e_ref, p_ref = _brute(lst, L, starts[b])
        assert rl[b].tolist() == r_ref and en[b].tolist() == e_ref and pr[b].item() == p_ref, (b, rl[b], r_ref, en[b], e_ref)


def test_strongest_paths_ties_and_empty():
    # two paths of equal product: 0 -(r1)-> 2 -(r0)-> 9 and 0 -(r0)-> 1 -(r0)-> 9; the last step's smaller head wins (1)
    lst = [(1, 0, 1, 2, 0.5), (1, 0, 0, 1, 0.5), (2, 2, 0, 9, 0.5), (2, 1, 0, 9, 0.5)]
    rd = _digraph([lst, []], 2)
    rl, en, pr = rd.strongest_paths()
    assert en[0].tolist() == [0, 1, 9] and rl[0].tolist() == [0, 0] and pr[0].item() == 0.25
    assert en[1].tolist() == [-1, -1, -1] and rl[1].tolist() == [-1, -1] and pr[1].item() == 0.0
    # same head, two relations: the smaller relation
    rd = _digraph([[(1, 3, 2, 4, 0.5), (1, 3, 1, 4, 0.5)]], 1)
    rl, en, pr = rd.strongest_paths()
    assert rl[0].tolist() == [1] and en[0].tolist() == [3, 4]
    # nothing at all
    rl, en, pr = _digraph([[], []], 3).strongest_paths()
    assert (rl == -1).all() and (en == -1).all() and (pr == 0).all()
