"""Cost of forecasting and explaining with the extrapolation model: one JSON line, on synthetic.make_extrapolation_shape("X") at
B = 64 with the (s, p) index over all data, for k = 1, 10, 100, 1000:
  - rg_segment_topk alone, on the logits and (query, entity) pairs of the batch's forward;
  - T_RED_GNN.predict (forward without the dense score matrix + rg_segment_topk) against the route the code offered before it, on the
    same tensors: _run(dense=True), the unvisited entries and the known objects masked to -inf (the known-object mask is built once,
    outside the timing), torch.topk;
and per hop of T_RED_GNN.explain (each row's own top forecast, min_alpha = 0) the rg_xexplain_count + rg_xexplain_emit pair next to the
same forward's rg_xlayer_fwd of that hop.
Times are device-event means over `reps` calls after a warm-up, taken `rounds` times alternating the contenders; the spread is
min..max over rounds.

    python tools/probe_extrap_predict.py [reps] [rounds]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd import extrapolation as X                        # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def mean_ms(f, reps):
    f()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def summary(ts):
    return dict(mean_ms=round(float(np.mean(ts)), 4), min_ms=round(float(np.min(ts)), 4), max_ms=round(float(np.max(ts)), 4))


def main():
    torch.cuda.set_device(0)
    data, n_ent, n_rel, gran = make_extrapolation_shape("X")
    sh = SHAPES["X"]

    class P:
        pass

    p = P()
    p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = (
        n_ent, n_rel, data, gran, sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda")
    torch.manual_seed(0)
    model = X.T_RED_GNN(p).cuda().eval()
    B = 64
    rng = np.random.default_rng(5)
    late = np.flatnonzero(data[:, 3] // gran >= 200)              # full 120-day windows
    q = data[np.sort(rng.choice(late, B, replace=False))]
    batch = X._Batch(q[:, 0], q[:, 1], q[:, 3])
    sp_index = X.known_objects_index(data, n_rel, False)
    dev = model.linear_classifier.weight.device

    with torch.no_grad():
        logits, _, nodes, _ = model._run(batch, dense=False)
    seg_ptr = torch.searchsorted(nodes[:, 0].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev))
    ent, logits = nodes[:, 1].contiguous(), logits.contiguous()
    q_key = torch.as_tensor(sp_index.query_keys(q[:, 0], q[:, 1], q[:, 3])).to(dev)
    known = model._index_on_device(sp_index, dev)
    known_mask = torch.zeros((B, n_ent), dtype=torch.bool)
    for b in range(B):
        known_mask[b, torch.as_tensor(sp_index.objects(q[b, 0], q[b, 1]).astype(np.int64))] = True
    known_mask = known_mask.to(dev)

    def dense_route(k):
        with torch.no_grad():
            _, _, nd, score_all = model._run(batch, dense=True)
            hide = torch.ones((B, n_ent), dtype=torch.bool, device=dev)
            hide[nd[:, 0].long(), nd[:, 1].long()] = False
            return torch.topk(score_all.masked_fill_(hide | known_mask, float("-inf")), k, dim=1)

    cases = []
    for k in (1, 10, 100, 1000):
        k_dense = min(k, n_ent)
        pred, ref = model.predict(batch, k=k, known=sp_index), dense_route(k_dense)
        n_cmp = min(k, k_dense)
        same = bool(torch.equal(pred.scores[:, :n_cmp], ref.values[:, :n_cmp]))          # (ids can differ inside a tie; the values cannot)
        t = {"rg_segment_topk": [], "predict": [], "dense_mask_topk": []}
        for _ in range(ROUNDS):
            t["rg_segment_topk"].append(mean_ms(lambda: engine.segment_topk(logits, ent, seg_ptr, k, q_key, known), REPS))
            t["predict"].append(mean_ms(lambda: model.predict(batch, k=k, known=sp_index), REPS))
            t["dense_mask_topk"].append(mean_ms(lambda: dense_route(k_dense), REPS))
        cases.append(dict(k=k, same_scores_as_dense_route=same, **{n: summary(v) for n, v in t.items()}))

    # explain: per hop the marking pair next to the forward's layer kernel of the same call
    engine.KERNEL_EVENTS, engine.EXPLAIN_EVENTS = [], []
    model.explain(batch)
    hops = {}
    for _ in range(ROUNDS):
        engine.KERNEL_EVENTS, engine.EXPLAIN_EVENTS = [], []
        for _ in range(REPS):
            rd = model.explain(batch)
        torch.cuda.synchronize()
        L = model.n_layer
        for i, (s, e, n_edges, n_new) in enumerate(engine.KERNEL_EVENTS):
            h = hops.setdefault(i % L + 1, dict(hop=i % L + 1, hop_edges=int(n_edges), fwd=[], xexplain=[]))
            h["fwd"].append(s.elapsed_time(e))
        for s, e, level, n_kept in engine.EXPLAIN_EVENTS:
            hops[level]["xexplain"].append(s.elapsed_time(e))
            hops[level]["digraph_edges"] = int(n_kept)
    engine.KERNEL_EVENTS = engine.EXPLAIN_EVENTS = None
    per_hop = []
    for l in sorted(hops):
        h = hops[l]
        rounds = lambda v: [float(np.mean(v[r * REPS:(r + 1) * REPS])) for r in range(ROUNDS)]
        per_hop.append(dict(hop=l, hop_edges=h["hop_edges"], digraph_edges=h["digraph_edges"], rg_xlayer_fwd=summary(rounds(h["fwd"])),
                            rg_xexplain_count_emit=summary(rounds(h["xexplain"]))))
    explain_ms = [mean_ms(lambda: model.explain(batch), REPS) for _ in range(ROUNDS)]
    lens = (seg_ptr[1:] - seg_ptr[:-1]).cpu().numpy()
    print(json.dumps(dict(
        probe="extrap_predict", shape="X", B=B, n_ent=n_ent, reps=REPS, rounds=ROUNDS, n_pairs=int(logits.numel()),
        segment_len_mean=round(float(lens.mean()), 1), segment_len_max=int(lens.max()),
        sp_list_mean=round(float(np.mean([len(sp_index.objects(s, r)) for s, r in zip(q[:, 0], q[:, 1])])), 1),
        topk=cases, explain=summary(explain_ms), explain_edges=int(rd.edges.shape[0]), per_hop=per_hop)))


if __name__ == "__main__":
    main()
