"""Cost of ranking one extrapolation batch on the device: one JSON line, on synthetic.make_extrapolation_shape("X") at B = 64, with
  - rg_segment_rank alone, on the softmax scores and (query, entity) pairs of the batch's forward (both filters);
  - T_RED_GNN.rank_batch (forward without the dense score matrix + rg_segment_rank) against the host route for the same batch:
    forward() (dense scores, the pairs copied to the host) + segment_rank_fil with the reference's sp2o / spt2o dictionaries.
Times are device-event means over `reps` calls after a warm-up, taken `rounds` times alternating the contenders (the host route's
Python time lies between its two events); the spread is min..max over rounds.

    python tools/probe_extrap_eval.py [reps] [rounds]
"""
import json
import os
import sys
from collections import defaultdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd import extrapolation as X                        # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape   # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 3


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
    # the split whose (s, p, t) objects are known: the rows from the first query's day on
    split = data[data[:, 3] >= q[0, 3] // gran * gran]
    sp_index, spt_index = X.known_objects_index(data, n_rel, False), X.known_objects_index(split, n_rel, True)
    sp2o, spt2o = defaultdict(list), defaultdict(list)           # utils.py:223-226,237-240
    for s, r, o, t in data.tolist():
        sp2o[(s, r)].append(o)
    for s, r, o, t in split.tolist():
        spt2o[(s, r, t)].append(o)
    sub, pre, ts = q[:, 0].tolist(), q[:, 1].tolist(), q[:, 3].tolist()

    def host_route():
        with torch.no_grad():
            _, (soft, ents) = model(batch)
        return X.segment_rank_fil(soft, ents, q[:, 2], sp2o, spt2o, sub, pre, ts)

    def device_route():
        return model.rank_batch(batch, q[:, 2], sp_index, spt_index)

    rb = device_route()
    host = X.segment_rank_fil(rb.soft, rb.nodes.long().cpu().numpy(), q[:, 2], sp2o, spt2o, sub, pre, ts)
    found = np.array(host[1])
    same = bool(np.array_equal(rb.found.cpu().numpy(), found) and np.array_equal(rb.rank.double().cpu().numpy(), host[0])
                and np.array_equal(rb.rank_fil.double().cpu().numpy(), host[2])
                and np.array_equal(rb.rank_fil_t.double().cpu().numpy()[found], host[3]))

    dev = rb.soft.device
    seg_ptr = torch.searchsorted(rb.nodes[:, 0].contiguous(), torch.arange(B + 1, dtype=torch.int32, device=dev))
    ent, soft = rb.nodes[:, 1].contiguous(), rb.soft.contiguous()
    target = torch.as_tensor(q[:, 2], dtype=torch.int32).to(dev)
    keys = [torch.as_tensor(ix.query_keys(q[:, 0], q[:, 1], q[:, 3])).to(dev) for ix in (sp_index, spt_index)]
    known = [model._index_on_device(ix, dev) for ix in (sp_index, spt_index)]
    kernel = [mean_ms(lambda: engine.segment_rank(soft, ent, seg_ptr, target, keys[0], known[0], keys[1], known[1]), 10 * REPS) for _ in range(ROUNDS)]

    t = {"rank_batch": [], "forward_plus_host_ranks": [], "forward": []}
    with torch.no_grad():
        for _ in range(ROUNDS):
            t["rank_batch"].append(mean_ms(device_route, REPS))
            t["forward_plus_host_ranks"].append(mean_ms(host_route, REPS))
            t["forward"].append(mean_ms(lambda: model(batch), REPS))
    lens = (seg_ptr[1:] - seg_ptr[:-1]).cpu().numpy()
    list_len = lambda ix, k: [len(ix.objects(*a)) for a in k]
    print(json.dumps(dict(
        probe="extrap_eval", shape="X", B=B, reps=REPS, rounds=ROUNDS, n_pairs=int(soft.numel()), segment_len_mean=round(float(lens.mean()), 1),
        segment_len_max=int(lens.max()), found=int(found.sum()),
        sp_list_mean=round(float(np.mean(list_len(sp_index, zip(sub, pre)))), 1), spt_list_mean=round(float(np.mean(list_len(spt_index, zip(sub, pre, ts)))), 1),
        device_ranks_equal_host_ranks=same, rg_segment_rank=summary(kernel), rank_batch=summary(t["rank_batch"]),
        forward_plus_host_ranks=summary(t["forward_plus_host_ranks"]), forward=summary(t["forward"]))))


if __name__ == "__main__":
    main()
