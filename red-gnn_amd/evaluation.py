"""Evaluation of the temporal interpolation model: loss, raw and filtered ranks of (head, relation, ?, time) queries.

    known = temporal_known_index(quads, n_rel + 1, n_time)             # (h, r, t): the time-aware filter
    known_static = temporal_static_known_index(quads, n_rel + 1)       # (h, r): the static filter
    metrics = model.evaluate(valid_quads, known, known_static)         # loss, hits1 / hits3 / hits10 / mrr / mr raw, _fil_t, _fil
    r = model.rank_batch(batch, tails, known, known_static)            # one batch, device tensors: r.logp, r.rank("fil_t"), ...

Replaces the validation loop of Temporal/interpolation/main.py:125-183, which per batch runs F.softmax over the dense [B, n_ent] score
matrix, nll_loss, three torch.topk, a full argsort and one .nonzero().item() host sync per query, and reports raw ranks only.  Here
the forward returns the logits of the visited (query, entity) pairs only (T_RED_GNN._run(dense=False)) and one HIP launch
(csrc/segment_eval.hip, rg_segment_eval) gives per query the loss term and the counts behind the three ranks; the entities a query
never reached score exactly 0 on the dense row and are counted arithmetically.
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import engine

KINDS = {"raw": "", "fil_t": "_fil_t", "fil": "_fil"}


@dataclass
class TemporalRanks:
    """Per query of a batch, device tensors [B].  ``logp`` float32: log(softmax(score row)[tail] + 1e-12), the term of main.py:146.
    ``visited`` bool: the forward reached the tail (otherwise it scores 0 and ranks among the zeros).  ``gt`` / ``eq`` int32: the
    number of entities scoring above the tail, and of other entities scoring exactly as it does; ``*_fil_t`` without the other tails
    known for (head, relation, time), ``*_fil`` without those known for (head, relation)."""
    logp: torch.Tensor
    visited: torch.Tensor
    gt: torch.Tensor
    eq: torch.Tensor
    gt_fil_t: torch.Tensor
    eq_fil_t: torch.Tensor
    gt_fil: torch.Tensor
    eq_fil: torch.Tensor

    def rank(self, kind="raw", ties="mean"):
        """float64 [B]: gt + eq / 2 + 1 (ties="mean", the convention of rg_rank and rg_segment_rank), gt + 1 ("lo") or gt + eq + 1
        ("hi") - the reference's argsort rank + 1 lies between the last two."""
        if kind not in KINDS:
            raise ValueError("rank: kind must be one of %s (got %r)" % (sorted(KINDS), kind))
        if ties not in ("mean", "lo", "hi"):
            raise ValueError("rank: ties must be 'mean', 'lo' or 'hi' (got %r)" % (ties,))
        gt, eq = getattr(self, "gt" + KINDS[kind]).double(), getattr(self, "eq" + KINDS[kind]).double()
        return gt + eq * {"mean": 0.5, "lo": 0.0, "hi": 1.0}[ties] + 1.0


def _check_known(known, who, name):
    if known is not None and (not isinstance(known, (tuple, list)) or len(known) != 3):
        raise ValueError("%s: %s must be a (keys, ptr, idx) triple (temporal_known_index / temporal_static_known_index)" % (who, name))


def _known_to(known, device):
    if known is None:
        return None
    return tuple(torch.as_tensor(x).to(device=device, dtype=dt).contiguous() for x, dt in zip(known, (torch.int64, torch.int64, torch.int32)))


def _tails(model, batch, tails, n, who):
    if tails is None:
        if "tail" not in batch:
            raise ValueError("%s: no tails given and the batch has no 'tail'" % who)
        tails = batch["tail"]
    a = (tails.detach().cpu().numpy() if torch.is_tensor(tails) else np.asarray(tails)).reshape(-1)
    if a.size and (a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer)):
        raise ValueError("%s: tails must hold integer ids (got dtype %s)" % (who, a.dtype))
    a = a.astype(np.int64)
    if len(a) != n:
        raise ValueError("%s: need one tail per head (got %d tails for %d heads)" % (who, len(a), n))
    if a.min() < 0 or a.max() >= model.n_ent:
        raise ValueError("%s: tail id out of range (n_ent=%d)" % (who, model.n_ent))
    return a


def _rank_validated(model, heads_h, rels_h, times_h, tails_h, known, known_static, device):
    """rank_batch on validated int64 host arrays [B] and indexes that are None or device triples: the ids and the queries' keys go to
    the device in one copy."""
    from .temporal import eval_semantics
    n = len(heads_h)
    key_hr = heads_h * (model.n_rel + 1) + rels_h
    ids = torch.as_tensor(np.stack([heads_h, rels_h, times_h, tails_h, key_hr * model.n_time + times_h, key_hr])).to(device)
    batch = {"head": ids[0], "relation": ids[1], "time": ids[2]}
    with torch.no_grad(), eval_semantics(model):
        logits, nodes = model._run(batch, "test", dense=False)
        # nodes are sorted by (query, entity): query q owns the pairs seg_ptr[q]:seg_ptr[q+1]
        seg_ptr = torch.searchsorted(nodes[:, 0].contiguous(), torch.arange(n + 1, dtype=torch.int32, device=device))
        logp, counts, visited = engine.segment_eval(logits.contiguous(), nodes[:, 1].contiguous(), seg_ptr, ids[3].to(torch.int32), model.n_ent,
                                                    None if known is None else ids[4], known,
                                                    None if known_static is None else ids[5], known_static)
    c = counts.unbind(1)
    return TemporalRanks(logp=logp, visited=visited.bool(), gt=c[0], eq=c[1], gt_fil_t=c[2], eq_fil_t=c[3], gt_fil=c[4], eq_fil=c[5])


def rank_batch_temporal(model, batch, tails=None, known=None, known_static=None):
    """T_RED_GNN.rank_batch (see there)."""
    from .temporal import batch_ids
    heads_h, rels_h, times_h = batch_ids(model, batch, "rank_batch")
    tails_h = _tails(model, batch, tails, len(heads_h), "rank_batch")
    _check_known(known, "rank_batch", "known")
    _check_known(known_static, "rank_batch", "known_static")
    device = model.linear_classifier.weight.device
    engine._require_gpu(device)
    return _rank_validated(model, heads_h, rels_h, times_h, tails_h, _known_to(known, device), _known_to(known_static, device), device)


def check_quads(model, quads, batch_size, who):
    """``quads`` as int64 [n, 4] = (head, rel, tail, time id) with ids inside the model's ranges; ValueError otherwise."""
    q = quads.detach().cpu().numpy() if torch.is_tensor(quads) else np.asarray(quads)
    if q.dtype == np.bool_ or not np.issubdtype(q.dtype, np.integer):
        raise ValueError("%s: quads must hold integer ids (got dtype %s)" % (who, q.dtype))
    if q.ndim != 2 or q.shape[1] != 4 or len(q) == 0:
        raise ValueError("%s: quads must be a non-empty int [n, 4] array of (head, rel, tail, time) (got shape %s)" % (who, q.shape))
    if isinstance(batch_size, (bool, np.bool_)) or not isinstance(batch_size, (int, np.integer)) or batch_size < 1:
        raise ValueError("%s: batch_size must be a positive integer (got %r)" % (who, batch_size))
    q = q.astype(np.int64)
    if (q[:, [0, 2]].min() < 0 or q[:, [0, 2]].max() >= model.n_ent or q[:, 1].min() < 0 or q[:, 1].max() > model.n_rel
            or q[:, 3].min() < 0 or q[:, 3].max() >= model.n_time):
        raise ValueError("%s: head / tail / relation / time id out of range (n_ent=%d, n_rel+1=%d, n_time=%d)"
                         % (who, model.n_ent, model.n_rel + 1, model.n_time))
    return q


def temporal_metrics(logp, visited, counts):
    """The metrics dict of T_RED_GNN.evaluate from per-query arrays: ``logp`` [n], ``visited`` [n] and ``counts`` {name: array [n]}
    with gt / eq, gt_fil_t / eq_fil_t, gt_fil / eq_fil.  Mean-tie ranks, sums in float64."""
    logp = np.asarray(logp, dtype=np.float64)
    n = len(logp)
    out = {"n": n, "loss": float(np.sum(-logp) / n), "unreached": float(np.sum(~np.asarray(visited, dtype=bool)) / n)}
    for sfx in KINDS.values():
        rank = np.asarray(counts["gt" + sfx], dtype=np.float64) + 0.5 * np.asarray(counts["eq" + sfx], dtype=np.float64) + 1.0
        out["hits1" + sfx], out["hits3" + sfx], out["hits10" + sfx] = (float(np.sum(rank <= k) / n) for k in (1, 3, 10))
        out["mrr" + sfx], out["mr" + sfx] = float(np.sum(1.0 / rank) / n), float(np.sum(rank) / n)
    return out


def evaluate_temporal(model, quads, known=None, known_static=None, batch_size=64, return_ranks=False):
    """T_RED_GNN.evaluate (see there)."""
    q = check_quads(model, quads, batch_size, "evaluate")
    _check_known(known, "evaluate", "known")
    _check_known(known_static, "evaluate", "known_static")
    device = model.linear_classifier.weight.device
    engine._require_gpu(device)
    known, known_static = _known_to(known, device), _known_to(known_static, device)        # to the device once, not per batch
    names = ("gt", "eq", "gt_fil_t", "eq_fil_t", "gt_fil", "eq_fil")
    parts = []
    for lo in range(0, len(q), int(batch_size)):
        b = q[lo:lo + int(batch_size)]
        r = _rank_validated(model, b[:, 0], b[:, 1], b[:, 3], b[:, 2], known, known_static, device)
        parts.append(torch.stack([r.logp.double(), r.visited.double()] + [getattr(r, k).double() for k in names]))
    host = torch.cat(parts, 1).cpu().numpy()                                               # the one host copy
    logp, visited = host[0], host[1] != 0
    counts = {k: host[2 + i].astype(np.int64) for i, k in enumerate(names)}
    out = temporal_metrics(logp, visited, counts)
    if return_ranks:
        per = dict(logp=logp, visited=visited, **counts)
        for kind, sfx in KINDS.items():
            per["rank" + sfx] = counts["gt" + sfx] + 0.5 * counts["eq" + sfx] + 1.0
        out["per_query"] = per
    return out
