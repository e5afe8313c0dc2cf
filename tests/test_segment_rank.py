"""CPU-only checks of the extrapolation evaluation: the C-ABI entry point rg_segment_rank is declared, bound and exported and refuses bad
arguments before any device work; known_objects_index against dictionaries built by the loops of the reference's get_sp2o / get_spt2o
(Temporal/extrapolation/utils.py:207-240); the argument checks of T_RED_GNN.evaluate and the metric formulas of main.py:413-463."""
import os
import re
import types
from collections import defaultdict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported():
    from red_gnn_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "redgnn.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+rg_segment_rank\s*\(", text)
    assert "rg_segment_rank" in _lib.SYMBOLS
    lib = _lib.lib()
    assert hasattr(lib, "rg_segment_rank") and len(lib.rg_segment_rank.argtypes) == 22


def test_bad_arguments_are_reported_before_any_device_work():
    """Non-zero return and a message; the pointers are made-up host addresses that a launch would fault on - none happens."""
    from red_gnn_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(64, dtype=np.int64)
    p = _lib.ptr(buf)

    def call(scores=p, ent=p, n_pairs=4, seg_ptr=p, target=p, batch=2, key_sp=None, sp=(None, None, None), n_sp=0, key_spt=None,
             spt=(None, None, None), n_spt=0, outs=(p, p, p, p)):
        return lib.rg_segment_rank(scores, ent, n_pairs, seg_ptr, 1, target, batch, key_sp, sp[0], sp[1], sp[2], n_sp, key_spt, spt[0], spt[1],
                                   spt[2], n_spt, outs[0], outs[1], outs[2], outs[3], None)

    for kw in (dict(seg_ptr=None), dict(target=None), dict(outs=(p, None, p, p)), dict(outs=(p, p, p, None))):
        assert call(**kw) != 0 and b"NULL" in lib.rg_last_error()
    for kw in (dict(scores=None), dict(ent=None)):
        assert call(**kw) != 0 and b"NULL pair array" in lib.rg_last_error()
    assert call(batch=0) != 0 and b"batch=0" in lib.rg_last_error()
    assert call(batch=-3) != 0 and b"batch=-3" in lib.rg_last_error()
    assert call(n_pairs=-1) != 0 and b"n_pairs=-1" in lib.rg_last_error()
    assert call(n_sp=-1) != 0 and b"n_keys=-1" in lib.rg_last_error()
    assert call(n_spt=-2) != 0 and b"n_keys" in lib.rg_last_error()
    assert call(n_sp=3, key_sp=p, sp=(p, None, p)) != 0 and b"NULL index array" in lib.rg_last_error()
    assert call(n_spt=3, key_spt=p, spt=(p, p, None)) != 0 and b"NULL index array" in lib.rg_last_error()
    assert call(n_sp=3, sp=(p, p, p)) != 0 and b"without per-query keys" in lib.rg_last_error()
    assert call(n_spt=3, spt=(p, p, p)) != 0 and b"without per-query keys" in lib.rg_last_error()


def _reference_dicts(data, split):
    """utils.py:223-226 and :237-240, literally."""
    sp2o, spt2o = defaultdict(list), defaultdict(list)
    for event in data:
        sp2o[(event[0], event[1])].append(event[2])
    for event in split:
        spt2o[(event[0], event[1], event[3])].append(event[2])
    return sp2o, spt2o


def test_known_objects_index_matches_the_reference_dictionaries():
    from red_gnn_amd import extrapolation as X
    rng = np.random.default_rng(11)
    n_ent, n_rel, n = 30, 4, 400
    data = np.stack([rng.integers(0, n_ent, n), rng.integers(0, n_rel, n), rng.integers(0, n_ent, n), rng.integers(0, 40, n) * 24], 1)
    data[50:60] = data[40:50]                                   # duplicate rows
    data[60] = data[61] = data[62]                              # ... one three times
    data = np.concatenate([data, [[n_ent - 1, n_rel - 1, 0, 39 * 24 + 7]]], 0)      # a key that occurs once, at the largest timestamp
    split = data[rng.choice(len(data), 150, replace=False)]     # a split: a subset of the data
    sp2o, spt2o = _reference_dicts(data, split)
    assert min(map(len, sp2o.values())) == 1 and max(map(len, sp2o.values())) > 3
    sp, spt = X.known_objects_index(data, n_rel, False), X.known_objects_index(split, n_rel, True)
    for ix, ref, with_time in ((sp, sp2o, False), (spt, spt2o, True)):
        keys, ptr, idx = ix
        assert keys.dtype == np.int64 and ptr.dtype == np.int64 and idx.dtype == np.int32
        assert len(keys) == len(ref) and np.all(np.diff(keys) > 0) and len(ptr) == len(keys) + 1 and ptr[0] == 0 and ptr[-1] == len(idx)
        assert ix.n_rel_rows == n_rel and ix.n_time == (int(split[:, 3].max()) + 1 if with_time else 0)
        for k, objs in ref.items():
            qk = ix.query_keys([k[0]], [k[1]], [k[2]] if with_time else None)[0]
            assert qk == ((k[0] * n_rel + k[1]) * ix.n_time + k[2] if with_time else k[0] * n_rel + k[1])
            i = int(np.searchsorted(keys, qk))
            assert keys[i] == qk
            assert np.array_equal(idx[ptr[i]:ptr[i + 1]], np.unique(objs))
            assert np.array_equal(ix.objects(*k), np.unique(objs))
    # what the dictionaries do not hold: an absent key, and ids outside the index's ranges, which must not alias another key
    absent = next((s, p) for s in range(n_ent) for p in range(n_rel) if (s, p) not in sp2o)
    assert len(sp.objects(*absent)) == 0
    assert sp.query_keys([3], [n_rel])[0] == -1 and sp.query_keys([-1], [0])[0] == -1
    assert spt.query_keys([3, 3, 3], [1, 1, 1], [spt.n_time, -1, spt.n_time - 1]).tolist()[:2] == [-1, -1]
    assert len(spt.objects(3, 1, spt.n_time + 5)) == 0
    # the layout of prediction.temporal_known_index
    from red_gnn_amd.prediction import temporal_known_index
    for a, b in zip(spt, temporal_known_index(split, n_rel, spt.n_time)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    empty = X.known_objects_index(np.zeros((0, 4), np.int64), n_rel, True)
    assert len(empty[0]) == 0 and empty[1].tolist() == [0] and len(empty[2]) == 0
    with pytest.raises(ValueError):
        X.known_objects_index(data.astype(np.float64), n_rel, False)
    with pytest.raises(ValueError):
        X.known_objects_index(data, n_rel - 1, False)


def test_evaluate_rejects_bad_queries_before_any_device_work():
    from red_gnn_amd import extrapolation as X
    model = types.SimpleNamespace(n_ent=20, n_rel_true=4, time_granularity=24, time_offset_list=np.zeros(12, np.int64))
    ev = lambda q, **kw: X.T_RED_GNN.evaluate(model, q, **kw)
    good = np.array([[1, 2, 3, 48], [0, 3, 19, 10 * 24 + 23]])
    for bad in (good.astype(np.float32), good.astype(bool), np.zeros((0, 4), np.int64), good[:, :3], good[0],
                good + [[20, 0, 0, 0]], good + [[0, 0, 1, 0]], good - [[2, 0, 0, 0]], good + [[0, 1, 0, 0]], good - [[0, 3, 0, 0]],
                good - [[0, 0, 0, 49]], good + [[0, 0, 0, 48]]):
        with pytest.raises(ValueError):
            ev(bad)
    for bs in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            ev(good, batch_size=bs)


def test_extrapolation_metrics_are_the_reference_formulas():
    """main.py:413-430 summed over batches, divided as :434-463 prints them; rank_fil_t holds the found queries only."""
    from red_gnn_amd import extrapolation as X
    rng = np.random.default_rng(5)
    n = 57
    found = rng.random(n) < 0.8
    rank = np.where(found, rng.integers(2, 60, n) / 2, 1e9)
    rank_fil = np.where(found, np.minimum(rank, rng.integers(2, 60, n) / 2), 1e9)
    rank_fil_t = np.minimum(rank, rng.integers(2, 60, n) / 2)[found]
    hits = dict.fromkeys(["h1", "h3", "h10", "h1f", "h3f", "h10f", "h1t", "h3t", "h10t", "found", "mr", "mrf", "mrr", "mrrf", "mrr_fil", "mrr_fil_t"], 0)
    at = 0
    for lo in range(0, n, 8):                                   # the reference's loop over batches
        r, f, rf = rank[lo:lo + 8], found[lo:lo + 8], rank_fil[lo:lo + 8]
        rt = rank_fil_t[at:at + int(f.sum())]
        at += int(f.sum())
        hits["h1"] += np.sum(r == 1); hits["h3"] += np.sum(r <= 3); hits["h10"] += np.sum(r <= 10)
        hits["h1f"] += np.sum(rf <= 1); hits["h3f"] += np.sum(rf <= 3); hits["h10f"] += np.sum(rf <= 10)
        hits["h1t"] += np.sum(rt <= 1); hits["h3t"] += np.sum(rt <= 3); hits["h10t"] += np.sum(rt <= 10)
        hits["found"] += np.sum(f); hits["mr"] += np.sum(r); hits["mrf"] += np.sum(r[f])
        hits["mrr"] += np.sum(1 / r); hits["mrrf"] += np.sum(1 / r[f]); hits["mrr_fil"] += np.sum(1 / rf); hits["mrr_fil_t"] += np.sum(1 / rt)
    m = X.extrapolation_metrics(rank, found, rank_fil, rank_fil_t)
    fc = hits["found"]
    want = dict(hits1=hits["h1"] / n, hits3=hits["h3"] / n, hits10=hits["h10"] / n, hits_inf=fc / n, mr=hits["mr"] / n, mrr=hits["mrr"] / n,
                hits1_fil=hits["h1f"] / n, hits3_fil=hits["h3f"] / n, hits10_fil=hits["h10f"] / n, mrr_fil=hits["mrr_fil"] / n,
                hits1_fil_t=hits["h1t"] / n, hits3_fil_t=hits["h3t"] / n, hits10_fil_t=hits["h10t"] / n, mrr_fil_t=hits["mrr_fil_t"] / n,
                hits1_found=hits["h1"] / fc, hits3_found=hits["h3"] / fc, hits10_found=hits["h10"] / fc, mr_found=hits["mrf"] / fc,
                mrr_found=hits["mrrf"] / fc)
    assert m["n"] == n and m["n_found"] == fc and set(m) == set(want) | {"n", "n_found"}
    for k, v in want.items():
        assert abs(m[k] - v) <= 1e-12 * max(1.0, abs(v)), k
    none = X.extrapolation_metrics(np.full(3, 1e9), np.zeros(3, bool), np.full(3, 1e9), np.zeros(0))
    assert none["hits_inf"] == 0 and none["mrr_fil_t"] == 0 and np.isnan(none["mrr_found"])
