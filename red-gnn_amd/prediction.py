"""Filtered top-k prediction: the k best new answers of queries (s, r, ?).

    pred = model.predict(subs, rels, k=10)              # exclude_known=True: no tail the loader's filter sets already hold
    pred.ids[b], pred.scores[b]                         # row b, score descending then entity id ascending; -1 / -inf past the end
    rd = model.explain(subs, rels, pred.ids[:, j])      # the r-digraph behind each row's j-th answer

The scores are forward()'s; the exclusion and the selection are one HIP launch (csrc/topk.hip, rg_topk) on the score matrix, with the
known answers as a sorted CSR over the query keys s * (2*n_rel + 1) + r (loader.known_index), copied to the device once.
Temporal interpolation: ``model.predict(batch, k, known=temporal_known_index(quads, n_rel + 1, n_time))`` with the batch dict of
forward; the keys are (head * n_rela_rows + rel) * n_time + time.
Temporal extrapolation: ``model.predict(X, k, known=known_objects_index(...))`` (extrapolation.py) selects among the entities each
query's window reaches (csrc/segment_topk.hip, rg_segment_topk) and also returns the softmax ``pred.prob``.
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
    ids, -inf past the end).  Tensors on the device that computed them.  ``prob`` (extrapolation only, None otherwise) float32 [B, k]:
    the per-query softmax over the entities the query's window reaches, 0 past the end."""
    ids: torch.Tensor
    scores: torch.Tensor
    prob: torch.Tensor = None


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


def temporal_known_index(quads, n_rela_rows, n_time):
    """Known-answer index of (head, relation, time) queries from quadruples int [n, 4] = (head, rel, tail, time id), in the layout of
    load_data.known_index_of: (keys int64 sorted and unique, ptr int64 [len(keys) + 1], idx int32) with key =
    (head * n_rela_rows + rel) * n_time + time and the tails of key i = idx[ptr[i]:ptr[i + 1]], ascending and unique."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    if len(q) and (q[:, 1].min() < 0 or q[:, 1].max() >= n_rela_rows or q[:, 3].min() < 0 or q[:, 3].max() >= n_time or q[:, [0, 2]].min() < 0):
        raise ValueError("temporal_known_index: relation / time id out of range (n_rela_rows=%d, n_time=%d)" % (n_rela_rows, n_time))
    key = (q[:, 0] * n_rela_rows + q[:, 1]) * n_time + q[:, 3]
    pairs = np.unique(np.stack([key, q[:, 2]], 1), axis=0) if len(q) else np.zeros((0, 2), np.int64)      # sorted by (key, tail)
    keys, first = np.unique(pairs[:, 0], return_index=True)
    ptr = np.append(first, len(pairs)).astype(np.int64)
    return keys.astype(np.int64), ptr, pairs[:, 1].astype(np.int32)


def temporal_static_known_index(quads, n_rela_rows):
    """The time-independent counterpart of temporal_known_index, for the static filter of T_RED_GNN.rank_batch / evaluate: the same
    layout with key = head * n_rela_rows + rel and the tails of (head, rel) at any time, ascending and unique."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 4)
    if len(q) and (q[:, 1].min() < 0 or q[:, 1].max() >= n_rela_rows or q[:, [0, 2]].min() < 0):
        raise ValueError("temporal_static_known_index: relation id outside 0..%d or a negative head / tail id" % (n_rela_rows - 1))
    key = q[:, 0] * n_rela_rows + q[:, 1]
    pairs = np.unique(np.stack([key, q[:, 2]], 1), axis=0) if len(q) else np.zeros((0, 2), np.int64)      # sorted by (key, tail)
    keys, first = np.unique(pairs[:, 0], return_index=True)
    ptr = np.append(first, len(pairs)).astype(np.int64)
    return keys.astype(np.int64), ptr, pairs[:, 1].astype(np.int32)


def predict_temporal(model, batch, k=10, known=None):
    """T_RED_GNN.predict (see there)."""
    from .temporal import batch_ids, eval_semantics
    device = model.linear_classifier.weight.device
    engine._require_gpu(device)
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)):
        raise ValueError("predict: k must be an integer in 1..%d (got %r)" % (K_MAX, k))
    k = int(k)
    if not 1 <= k <= K_MAX:
        raise ValueError("predict: k=%d not in 1..%d" % (k, K_MAX))
    heads_h, rels_h, times_h = batch_ids(model, batch, "predict")
    with torch.no_grad(), eval_semantics(model):
        scores = model._run(batch, "test")
        q_key = None
        if known is not None:
            if len(known) != 3:
                raise ValueError("predict: known must be the (keys, ptr, idx) triple of temporal_known_index")
            known = tuple(torch.as_tensor(x).to(device=device, dtype=dt).contiguous()
                          for x, dt in zip(known, (torch.int64, torch.int64, torch.int32)))
            q_key = torch.as_tensor((heads_h * (model.n_rel + 1) + rels_h) * model.n_time + times_h, dtype=torch.int64).to(device)
        idx, val = engine.topk(scores.contiguous(), k, q_key, known)
    return Prediction(ids=idx.long(), scores=val)

