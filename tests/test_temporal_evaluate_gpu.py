"""T_RED_GNN.rank_batch / evaluate (temporal interpolation) on the GPU against tests/segment_eval_ref.py applied to the rows of
forward's dense score matrix: counts exact, logp within the project's stated tolerance (README: rtol 1e-4, atol 2e-5)."""
import functools

import numpy as np
import pytest
import torch

from tests import layer_ref as LR
from tests import segment_eval_ref as R
from tests import temporal_ref as TR

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5
NAMES = ("gt", "eq", "gt_fil_t", "eq_fil_t", "gt_fil", "eq_fil")


@functools.lru_cache(maxsize=None)
def _setup(B=20):
    """As test_temporal_predict_gpu._setup: 3 layers, d = 32; the last query's head has only its identity edge.  With the per-query
    reference (logp float64, counts, visited) of the model's own dense score rows, computed once."""
    from red_gnn_amd.prediction import temporal_known_index, temporal_static_known_index
    c = LR._temporal_case("predict", seed=4, B=B, m=600)
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, 3, 32, 5, "relu")
    quads = c.quads[:B].copy()
    quads[-1] = (c.n_ent - 1, 3, 7, 1)                          # a head with its identity edge only: one visited pair, the tail unreached
    known = temporal_known_index(c.quads, c.n_rela_rows, c.n_time)
    known_static = temporal_static_known_index(c.quads, c.n_rela_rows)
    batch = {"head": quads[:, 0], "relation": quads[:, 1], "time": quads[:, 3], "tail": quads[:, 2]}
    with torch.no_grad():
        scores = model(batch, mode="test").cpu().numpy()
    key_hr = quads[:, 0] * c.n_rela_rows + quads[:, 1]
    ref = [R.row_eval(scores[b], int(quads[b, 2]), R.list_of(known, key_hr[b] * c.n_time + quads[b, 3]), R.list_of(known_static, key_hr[b]))
           for b in range(B)]
    logp, counts = np.array([r[0] for r in ref]), np.stack([r[1] for r in ref])
    return c, model, quads, batch, known, known_static, scores, logp, counts


def _assert_ranks(r, logp, counts, scores, tails):
    for t, dt in [(r.logp, torch.float32), (r.visited, torch.bool)] + [(getattr(r, k), torch.int32) for k in NAMES]:
        assert t.is_cuda and t.dtype == dt and t.shape == (len(tails),) and not t.requires_grad
    got = torch.stack([getattr(r, k) for k in NAMES], 1).cpu().numpy()
    assert np.array_equal(got, counts), (got, counts)
    err = np.abs(r.logp.double().cpu().numpy() - logp)
    print("rank_batch: max |logp - ref| = %.3g" % err.max())
    assert np.all(err <= ATOL + RTOL * np.abs(logp))
    assert np.array_equal(r.visited.cpu().numpy(), scores[np.arange(len(tails)), tails] != 0)


def test_rank_batch_against_the_dense_rows():
    c, model, quads, batch, known, known_static, scores, logp, counts = _setup()
    r = model.rank_batch(batch, None, known, known_static)       # tails from batch["tail"]
    _assert_ranks(r, logp, counts, scores, quads[:, 2])
    assert not r.visited[-1] and r.visited.sum() >= 10
    # the static list of (h, r) holds the time-aware list of (h, r, t): it hides no less, and somewhere it hides something
    assert np.all(counts[:, 4:] <= counts[:, 2:4]) and np.all(counts[:, 2:4] <= counts[:, :2]) and np.any(counts[:, 4:].sum(1) < counts[:, :2].sum(1))
    assert np.array_equal(r.rank("fil_t").cpu().numpy(), counts[:, 2] + 0.5 * counts[:, 3] + 1)
    # other tails than the batch's, and no filter: the raw counts three times
    tails = np.roll(quads[:, 2], 3)
    ref = [R.row_eval(scores[b], int(tails[b])) for b in range(len(tails))]
    r2 = model.rank_batch({k: batch[k] for k in ("head", "relation", "time")}, torch.as_tensor(tails))
    _assert_ranks(r2, np.array([x[0] for x in ref]), np.stack([x[1] for x in ref]), scores, tails)
    assert torch.equal(r2.gt, r2.gt_fil) and torch.equal(r2.eq, r2.eq_fil_t)


def test_run_without_the_dense_matrix_is_forward_bit_for_bit():
    c, model, quads, batch, *_ , scores, _, _ = _setup()
    with torch.no_grad():
        result, nodes = model._run(batch, "test", dense=False)
        dense = model._run(batch, "test")
    assert result.dtype == torch.float32 and nodes.dtype == torch.int32 and nodes.shape == (result.numel(), 2)
    scattered = torch.zeros(len(quads), c.n_ent, device="cuda")
    scattered[nodes[:, 0].long(), nodes[:, 1].long()] = result
    assert torch.equal(scattered, dense) and np.array_equal(dense.cpu().numpy(), scores)
    key = nodes[:, 0].long() * c.n_ent + nodes[:, 1].long()
    assert bool((key[1:] > key[:-1]).all())                       # sorted by (query, entity): what rank_batch's segments rely on


def test_evaluate_batches_index_forms_and_training_flags():
    from red_gnn_amd.evaluation import temporal_metrics
    c, model, quads, batch, known, known_static, scores, logp, counts = _setup()
    visited = scores[np.arange(len(quads)), quads[:, 2]] != 0
    want = temporal_metrics(logp, visited, {k: counts[:, i] for i, k in enumerate(NAMES)})
    # ... which is, written out for the raw and the time-aware ranks:
    rank, rank_t = counts[:, 0] + 0.5 * counts[:, 1] + 1, counts[:, 2] + 0.5 * counts[:, 3] + 1
    assert want["n"] == 20 and abs(want["mrr"] - np.mean(1 / rank)) < 1e-15 and abs(want["hits3_fil_t"] - np.mean(rank_t <= 3)) < 1e-15
    assert abs(want["loss"] + logp.mean()) < 1e-15 and want["unreached"] == np.mean(~visited) > 0

    def close(m, want=want):
        assert m.keys() == want.keys()
        for k, v in want.items():                                 # everything but the loss is a function of exact integers
            assert abs(m[k] - v) <= ((ATOL + RTOL * abs(v)) if k == "loss" else 1e-12), (k, m[k], v)

    m8 = model.evaluate(quads, known, known_static, batch_size=8, return_ranks=True)        # 8 + 8 + 4
    per = m8.pop("per_query")
    close(m8)
    assert np.array_equal(np.stack([per[k] for k in NAMES], 1), counts) and np.array_equal(per["visited"], visited)
    assert per["logp"].dtype == np.float64 and np.array_equal(per["rank_fil_t"], rank_t) and np.array_equal(per["rank"], rank)
    m20 = model.evaluate(quads, known, known_static, batch_size=20, return_ranks=True)
    per20 = m20.pop("per_query")
    # "The same result" at another batch size, deliberately stated as: every count, rank and visited flag exactly equal, logp and the
    # loss within the stated tolerance.  rg_segment_eval itself is bitwise batch-independent (tests/test_segment_eval_gpu.py), but the
    # forward's GEMMs are not promised to give a query's logits the same last bit at 8 and at 20 rows, and logp inherits that.
    close(m20, m8)
    assert all(np.array_equal(per[k], per20[k]) for k in per if k != "logp") and np.allclose(per["logp"], per20["logp"], rtol=RTOL, atol=ATOL)
    dev = lambda ix: tuple(torch.as_tensor(x).cuda() for x in ix)
    assert model.evaluate(torch.as_tensor(quads), dev(known), dev(known_static), batch_size=8) == m8      # the same launches on the same inputs
    raw = model.evaluate(quads, batch_size=8)
    assert raw["mrr_fil"] == raw["mrr_fil_t"] == raw["mrr"] == m8["mrr"] and raw["mr_fil"] == raw["mr"] and raw["loss"] == m8["loss"]
    was = model.training
    model.train()
    model.dropout.p = 0.5
    try:
        again = model.evaluate(quads, known, known_static, batch_size=8)
        assert model.training and model.dropout.training
    finally:
        model.dropout.p = 0.0
        model.train(was)
    assert again == m8
