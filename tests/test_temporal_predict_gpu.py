"""T_RED_GNN.predict on the MI355X (-m gpu): filtered top-k ids and scores against masked_fill_ of the known tails plus a stable sort
(score descending, id ascending) of forward's scores."""
import numpy as np
import pytest
import torch

from tests import layer_ref as LR
from tests import temporal_ref as TR

pytestmark = pytest.mark.gpu


def _setup(B=9):
    from red_gnn_amd.prediction import temporal_known_index
    c = LR._temporal_case("predict", seed=4, B=B, m=600)
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, 3, 32, 5, "relu")
    heads, rels, times = c.quads[:B, 0].copy(), c.quads[:B, 1].copy(), c.quads[:B, 3].copy()      # queries whose keys are in the index
    heads[-1], rels[-1], times[-1] = c.n_ent - 1, 3, 1              # ... and one whose key is absent (an entity with its identity edge only)
    known = temporal_known_index(c.quads, c.n_rela_rows, c.n_time)
    return c, model, {"head": heads, "relation": rels, "time": times}, known


def _expected(scores, batch, known, k, c):
    s = scores.clone()
    if known is not None:
        keys, ptr, idx = known
        for b in range(s.shape[0]):
            key = (int(batch["head"][b]) * c.n_rela_rows + int(batch["relation"][b])) * c.n_time + int(batch["time"][b])
            i = np.searchsorted(keys, key)
            if i < len(keys) and keys[i] == key:
                s[b].masked_fill_(torch.zeros(s.shape[1], dtype=torch.bool).index_fill_(0, torch.as_tensor(idx[ptr[i]:ptr[i + 1]]).long(), True),
                                  float("nan"))
    ids = torch.full((s.shape[0], k), -1, dtype=torch.int64)
    val = torch.full((s.shape[0], k), float("-inf"))
    for b in range(s.shape[0]):
        left = torch.nonzero(~torch.isnan(s[b])).reshape(-1)
        order = left[torch.sort(s[b, left], descending=True, stable=True).indices][:k]      # stable: ids ascending among equal scores
        ids[b, :len(order)] = order
        val[b, :len(order)] = s[b, order]
    return ids, val


@pytest.mark.parametrize("k", [1, 10, 200])
@pytest.mark.parametrize("with_known", [True, False])
def test_predict_against_masked_stable_sort(k, with_known):
    c, model, batch, known = _setup()
    with torch.no_grad():
        scores = model(batch, mode="test").cpu()
    kn = known if with_known else None
    pred = model.predict(batch, k=k, known=kn)
    ids, val = _expected(scores, batch, kn, k, c)
    assert pred.ids.dtype == torch.int64 and pred.ids.shape == (9, k) and pred.scores.dtype == torch.float32
    assert torch.equal(pred.ids.cpu(), ids) and torch.equal(pred.scores.cpu(), val)
    if with_known:
        keys = (batch["head"] * c.n_rela_rows + batch["relation"]) * c.n_time + batch["time"]
        assert np.isin(keys[:-1], known[0]).all() and not np.isin(keys[-1], known[0])
        if k == c.n_ent:                                                 # k = n_ent: the known tails leave padding behind
            assert (pred.ids[:-1, -1] == -1).all() and torch.isinf(pred.scores[:-1, -1]).all() and (pred.ids[-1] >= 0).all()
        dev = tuple(torch.as_tensor(x).cuda() for x in known)            # the same index as device tensors
        again = model.predict(batch, k=k, known=dev)
        assert torch.equal(again.ids, pred.ids) and torch.equal(again.scores, pred.scores)
    elif k == c.n_ent:
        assert (pred.ids >= 0).all()


def test_explain_of_the_top_answer_and_arguments():
    c, model, batch, known = _setup()
    pred = model.predict(batch, k=3, known=known)
    rd = model.explain(batch, pred.ids[:, 0])
    assert torch.equal(rd.score, pred.scores[:, 0])
    assert rd.reached[pred.scores[:, 0] != 0].all()
    for bad in (0, 1025, True, 2.0, None):
        with pytest.raises(ValueError):
            model.predict(batch, k=bad)
    with pytest.raises(ValueError):
        model.predict({"head": [c.n_ent], "relation": [0], "time": [0]}, k=1)
    with pytest.raises(ValueError):
        model.predict({"head": [0], "relation": [0], "time": [c.n_time]}, k=1)
    with pytest.raises(ValueError):
        model.predict(batch, k=1, known=known[:2])
    was = model.training
    model.train()
    model.dropout.p = 0.5
    again = model.predict(batch, k=3, known=known)
    assert model.training
    model.train(was)
    assert torch.equal(again.ids, pred.ids) and torch.equal(again.scores, pred.scores)
