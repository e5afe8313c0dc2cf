"""Filtered top-k prediction: the k best new answers of queries (s, r, ?).

    pred = model.predict(subs, rels, k=10)              # exclude_known=True: no tail the loader's filter sets already hold
    pred.ids[b], pred.scores[b]                         # row b, score descending then entity id ascending; -1 / -inf past the end
    rd = model.explain(subs, rels, pred.ids[:, j])      # the r-digraph behind each row's j-th answer

The scores are forward()'s; the exclusion and the selection are one HIP launch (csrc/topk.hip, rg_topk) on the score matrix, with the
known answers as a sorted CSR over the query keys s * (2*n_rel + 1) + r (loader.known_index), copied to the device once.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import engine
from .explain import _ids

K_MAX = 1024


@dataclass
class Prediction:
    """ids int64 [B, k] (entity ids, -1 where the row has fewer than k candidates), scores float32 [B, k] (forward's scores of those
    ids, -inf past the end).  Tensors on the device that computed them."""
    ids: torch.Tensor
    scores: torch.Tensor


def _known_on_device(loader, mode, device):
    """loader.known_index(mode) as device tensors, copied once per loader, mode and device (held by the loader)."""
    cache = loader.__dict__.setdefault("_known_index_dev", {})
    key = (mode, str(device))
    if key not in cache:
        cache[key] = tuple(torch.as_tensor(a).to(device) for a in loader.known_index(mode))
    return cache[key]


def predict(model, subs, rels, k=10, exclude_known=True, mode="test"):
    """RED_GNN_trans.predict (see there)."""
    device = model.W_final.weight.device
    engine._require_gpu(device)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError("predict: k must be an integer in 1..%d (got %r)" % (K_MAX, k))
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError("predict: k=%d not in 1..%d" % (k, K_MAX))
    subs_h, rels_h = _ids(subs, "subs"), _ids(rels, "rels")
    n = len(subs_h)
    if n == 0 or len(rels_h) != n:
        raise ValueError("predict: need one relation per subject and at least one row (got %d subjects, %d relations)" % (n, len(rels_h)))
    n_ent = model.loader.graph_for(mode).n_ent
    n_rows = 2 * model.n_rel + 1
    if subs_h.min() < 0 or subs_h.max() >= n_ent or rels_h.min() < 0 or rels_h.max() >= n_rows:
        raise ValueError("query subject / relation id out of range (n_ent=%d, 2*n_rel+1=%d)" % (n_ent, n_rows))
    with torch.no_grad():
        scores = model._run(subs_h, rels_h, mode, eval_mode=True)
        known, q_key = None, None
        if exclude_known:
            known = _known_on_device(model.loader, mode, device)
            q_key = torch.as_tensor(subs_h * n_rows + rels_h, dtype=torch.int64).to(device)
        idx, val = engine.topk(scores.contiguous(), k, q_key, known)
    return Prediction(ids=idx.long(), scores=val)
