"""CPU-only checks of the interpolation evaluation: the numpy reference of rg_segment_eval (tests/segment_eval_ref.py) against the
literal torch sequence of the reference's validation loop, temporal_static_known_index, the C-ABI entry point declared and bound,
the argument checks of T_RED_GNN.rank_batch / evaluate - which run before any device work (the model here is a namespace with the
attributes the checks read: nothing else may be touched) - and the probe's --help."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import segment_eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_numpy_reference_agrees_with_the_torch_sequence():
    """On the dense float64 rows of the edge case: logp within 1e-12 of F.softmax / nll_loss, and the argsort rank + 1 inside
    [gt + 1, gt + eq + 1] for every row.  The row with a NaN score has NaN probabilities throughout - its argsort says nothing about
    the logits - so there only the NaN of logp is compared."""
    c = R.edge_case()
    B = len(c["target"])
    x = np.stack([R.dense_row(c["scores"][c["seg_ptr"][q]:c["seg_ptr"][q + 1]], c["ent"][c["seg_ptr"][q]:c["seg_ptr"][q + 1]], R.N_ENT)
                  for q in range(B)])
    logp, rank, hits = R.torch_reference(x.astype(np.float64), c["target"])
    ref_logp, counts, visited = c["ref"]
    nan = np.isnan(ref_logp)
    assert nan.tolist() == [q == R.WITH_NAN for q in range(B)] and np.array_equal(np.isnan(logp), nan)
    assert np.max(np.abs(logp[~nan] - ref_logp[~nan])) <= 1e-12
    lo, hi = counts[:, 0] + 1, counts[:, 0] + counts[:, 1] + 1
    assert np.all((lo <= rank) & (rank <= hi) | nan), (rank, lo, hi)
    assert np.any(hi - lo > 5000)                                 # ties with the zeros: the reference's rank is one of thousands of places
    # hits@k of the batch lie between the counts by the best and by the worst tied place
    for k, h in zip((1, 3, 10), hits):
        assert np.sum(hi[~nan] <= k) <= h <= np.sum(lo[~nan] <= k) + int(nan.sum())
    assert visited.tolist() == [c["where"][q] is not None for q in range(B)]
    # the raw counts do not depend on the lists, and filtering can only lower them
    again = R.segment_eval(c["scores"], c["ent"], c["seg_ptr"], c["target"], R.N_ENT)
    assert np.array_equal(again[1][:, :2], counts[:, :2]) and np.array_equal(again[1][:, 2:4], counts[:, :2])
    assert np.all(counts[:, 2:] <= np.tile(counts[:, :2], 2))


def test_static_known_index_layout():
    from red_gnn_amd.prediction import temporal_known_index, temporal_static_known_index
    rng = np.random.default_rng(3)
    n_ent, n_rows, n_time = 30, 7, 5
    quads = np.stack([rng.integers(0, n_ent, 400), rng.integers(0, n_rows, 400), rng.integers(0, n_ent, 400), rng.integers(0, n_time, 400)], 1)
    quads[10:14] = quads[9]                                       # duplicates
    keys, ptr, idx = temporal_static_known_index(quads, n_rows)
    assert keys.dtype == np.int64 and ptr.dtype == np.int64 and idx.dtype == np.int32
    assert np.all(np.diff(keys) > 0) and len(ptr) == len(keys) + 1 and ptr[0] == 0 and ptr[-1] == len(idx)
    want = {}
    for h, r, t, _ in quads.tolist():
        want.setdefault(h * n_rows + r, set()).add(t)
    assert keys.tolist() == sorted(want)
    for i, k in enumerate(keys.tolist()):
        assert idx[ptr[i]:ptr[i + 1]].tolist() == sorted(want[k])
    # the static list of (h, r) is the union of the time-aware lists of (h, r, t)
    tk, tp, ti = temporal_known_index(quads, n_rows, n_time)
    for i, k in enumerate(tk.tolist()):
        assert set(ti[tp[i]:tp[i + 1]].tolist()) <= want[k // n_time]
    e = temporal_static_known_index(np.zeros((0, 4), np.int64), n_rows)
    assert len(e[0]) == 0 and e[1].tolist() == [0] and len(e[2]) == 0
    for bad in ([[0, n_rows, 1, 0]], [[0, -1, 1, 0]], [[-1, 0, 1, 0]], [[0, 0, -1, 0]]):
        with pytest.raises(ValueError):
            temporal_static_known_index(np.array(bad), n_rows)


def test_entry_point_is_declared_and_bound():
    from red_gnn_amd import _lib, engine
    header = open(os.path.join(ROOT, "include", "redgnn.h")).read()
    assert re.search(r"\bint rg_segment_eval\(", header) and "rg_segment_eval" in _lib.SYMBOLS
    assert os.path.exists(os.path.join(ROOT, "red-gnn_amd", "csrc", "segment_eval.hip")) and callable(engine.segment_eval)


def _model():
    return types.SimpleNamespace(n_ent=20, n_rel=6, n_time=12)


def _batch(head, rel, time, **kw):
    return dict(head=np.asarray(head), relation=np.asarray(rel), time=np.asarray(time), **kw)


BAD_BATCHES = [
    _batch([1.0, 2.0], [0, 1], [3, 4]),              # float ids
    _batch([1, 2], [0.5, 1.0], [3, 4]),
    _batch([1, 2], [0, 1], [3.0, 4.0]),
    _batch([True, False], [0, 1], [3, 4]),
    _batch([1, 2], [0], [3, 4]),                     # lengths
    _batch([1, 2], [0, 1], [3]),
    _batch([], [], []),
    _batch([1, 20], [0, 1], [3, 4]),                 # ranges
    _batch([-1, 2], [0, 1], [3, 4]),
    _batch([1, 2], [0, 7], [3, 4]),
    _batch([1, 2], [-1, 1], [3, 4]),
    _batch([1, 2], [0, 1], [3, 12]),
    _batch([1, 2], [0, 1], [-1, 4]),
    dict(head=np.array([1, 2]), relation=np.array([0, 1])),
]
KNOWN = (np.array([3], np.int64), np.array([0, 1], np.int64), np.array([2], np.int32))


def test_rank_batch_rejects_bad_arguments_before_any_device_work():
    from red_gnn_amd.temporal import T_RED_GNN
    good = _batch([1, 2], [0, 6], [0, 11])
    for bad in BAD_BATCHES:
        with pytest.raises(ValueError):
            T_RED_GNN.rank_batch(_model(), bad, [0, 1])
    for tails in ([0], [0, 1, 2], [0, 20], [-1, 0], [0.0, 1.0], [True, False], None):      # None: the batch has no 'tail'
        with pytest.raises(ValueError):
            T_RED_GNN.rank_batch(_model(), good, tails)
    with pytest.raises(ValueError):
        T_RED_GNN.rank_batch(_model(), dict(good, tail=np.array([0, 20])))
    for name in ("known", "known_static"):
        for bad in (KNOWN[:2], KNOWN + KNOWN[:1], 5):
            with pytest.raises(ValueError):
                T_RED_GNN.rank_batch(_model(), good, [0, 1], **{name: bad})
    for args in ((good, [0, 19]), (dict(good, tail=np.array([0, 19])),), (good, torch.tensor([0, 19]), KNOWN, KNOWN)):
        with pytest.raises(AttributeError):          # a good call gets past the checks (the namespace has no parameters)
            T_RED_GNN.rank_batch(_model(), *args)


def test_evaluate_rejects_bad_arguments_before_any_device_work():
    from red_gnn_amd.temporal import T_RED_GNN
    good = np.array([[1, 0, 0, 0], [2, 6, 19, 11]])
    bad_quads = [good.astype(np.float64), good.astype(bool), good[:, :3], good.reshape(-1), good[:0],
                 [[20, 0, 0, 0]], [[-1, 0, 0, 0]], [[0, 7, 0, 0]], [[0, -1, 0, 0]], [[0, 0, 20, 0]], [[0, 0, -1, 0]], [[0, 0, 0, 12]],
                 [[0, 0, 0, -1]]]
    for bad in bad_quads:
        with pytest.raises(ValueError):
            T_RED_GNN.evaluate(_model(), np.asarray(bad))
    for bs in (0, -1, 2.0, True, None, "8"):
        with pytest.raises(ValueError):
            T_RED_GNN.evaluate(_model(), good, batch_size=bs)
    for name in ("known", "known_static"):
        with pytest.raises(ValueError):
            T_RED_GNN.evaluate(_model(), good, **{name: KNOWN[:2]})
    for kw in ({}, dict(known=KNOWN, known_static=KNOWN, batch_size=1, return_ranks=True), dict(quads=torch.as_tensor(good))):
        with pytest.raises(AttributeError):
            T_RED_GNN.evaluate(_model(), **dict(dict(quads=good), **kw))


def test_ranks_result_type():
    from red_gnn_amd.evaluation import TemporalRanks, temporal_metrics
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    r = TemporalRanks(logp=torch.tensor([-1.0, -2.0]), visited=torch.tensor([True, False]), gt=i32(0, 4), eq=i32(0, 3), gt_fil_t=i32(0, 2),
                      eq_fil_t=i32(0, 1), gt_fil=i32(0, 1), eq_fil=i32(0, 0))
    assert r.rank().dtype == torch.float64 and r.rank().tolist() == [1.0, 6.5]
    assert r.rank("raw", "lo").tolist() == [1.0, 5.0] and r.rank("raw", "hi").tolist() == [1.0, 8.0]
    assert r.rank("fil_t").tolist() == [1.0, 3.5] and r.rank("fil", "hi").tolist() == [1.0, 2.0]
    for bad in (dict(kind="filtered"), dict(ties="min"), dict(kind=None)):
        with pytest.raises(ValueError):
            r.rank(**bad)
    m = temporal_metrics(r.logp.numpy(), r.visited.numpy(), {k: getattr(r, k).numpy() for k in ("gt", "eq", "gt_fil_t", "eq_fil_t", "gt_fil", "eq_fil")})
    assert m["n"] == 2 and m["loss"] == 1.5 and m["unreached"] == 0.5
    assert m["hits1"] == 0.5 and m["hits10"] == 1.0 and m["mr"] == 3.75 and abs(m["mrr"] - (1 + 1 / 6.5) / 2) < 1e-15
    assert m["hits3_fil_t"] == 0.5 and m["hits3_fil"] == 1.0 and m["mr_fil"] == 1.5


def test_probe_answers_help():
    r = subprocess.run([sys.executable, os.path.join("tools", "probe_temporal_eval.py"), "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "rg_segment_eval" in r.stdout and "C5" in r.stdout
