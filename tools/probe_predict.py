"""Cost of filtered top-k prediction: one JSON line with
  - rg_topk against masked_fill_ + torch.topk on the same device tensors (the score matrix of a C2 forward at B = 1024, its rows'
    known answers excluded; k = 1, 10, 100, 1000), and on a 123 k-entity row width at B = 64 (seeded normal scores, 20 known per row);
  - RED_GNN_trans.predict(k = 10) against forward() at C2, B = 1024 (both replayed from a captured graph after warm-up).
Times are device-event means over `reps` calls, taken `rounds` times alternating the contenders; the spread is min..max over rounds.

    python tools/probe_predict.py [reps] [rounds]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.load_data import DataLoader                      # noqa: E402
from red_gnn_amd.models import RED_GNN_trans                      # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_shape              # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 50
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def mean_ms(f, reps=REPS):
    f()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def contest(fs):
    """{name: [ms per round]}, the contenders alternating inside every round."""
    out = {n: [] for n in fs}
    for _ in range(ROUNDS):
        for n, f in fs.items():
            out[n].append(mean_ms(f))
    return out


def summary(ts):
    return dict(mean_ms=round(float(np.mean(ts)), 4), min_ms=round(float(np.min(ts)), 4), max_ms=round(float(np.max(ts)), 4))


def mask_of(q_key, index, B, n_ent, device):
    keys, ptr, idx = index
    mask = torch.zeros((B, n_ent), dtype=torch.bool)
    for b, q in enumerate(q_key.tolist()):
        i = np.searchsorted(keys, q)
        if i < len(keys) and keys[i] == q:
            mask[b, torch.as_tensor(idx[ptr[i]:ptr[i + 1]].astype(np.int64))] = True
    return mask.to(device)


def topk_cases(scores, q_key_h, index_h, ks, label):
    B, n_ent = scores.shape
    dev = scores.device
    q_key = torch.as_tensor(q_key_h).to(dev)
    known = tuple(torch.as_tensor(a).to(dev) for a in index_h)
    mask = mask_of(q_key_h, index_h, B, n_ent, dev)
    work = scores.clone()
    res = []
    for k in ks:
        a_ids, _ = engine.topk(scores, k, q_key, known)
        ref = torch.topk(scores.masked_fill(mask, float("-inf")), k, dim=1)
        agree = bool(torch.equal(torch.sort(a_ids.long(), 1)[0], torch.sort(ref.indices, 1)[0]))   # (no ties at the cut on these rows)

        def ours():
            engine.topk(scores, k, q_key, known)

        def torch_path():
            work.masked_fill_(mask, float("-inf"))
            torch.topk(work, k, dim=1)
        t = contest({"rg_topk": ours, "masked_fill_topk": torch_path})
        res.append(dict(case=label, B=B, n_ent=n_ent, k=k, rg_topk=summary(t["rg_topk"]),
                        masked_fill_topk=summary(t["masked_fill_topk"]), same_sets_as_torch=agree))
    return res


def main():
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    shape = SHAPES["C2"]
    kg = make_shape("C2")
    loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test),
                        verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = shape["n_layer"], shape["hidden_dim"], shape["attn_dim"], kg.n_rel, "relu", 0.0

    torch.manual_seed(0)
    model = RED_GNN_trans(P, loader).cuda().eval()
    B = 1024
    q = np.arange(B) % loader.n_test
    subs = np.array([loader.test_q[i][0] for i in q])
    rels = np.array([loader.test_q[i][1] for i in q])
    with torch.no_grad():
        for _ in range(3):                      # the third call captures the graph
            scores = model(subs, rels, mode="test")
            model.predict(subs, rels, k=10)
        t = contest({"forward": lambda: model(subs, rels, mode="test"), "predict": lambda: model.predict(subs, rels, k=10)})
    index = loader.known_index("test")
    q_key = subs.astype(np.int64) * (2 * loader.n_rel + 1) + rels
    known_per_row = float(np.mean([len(loader.filters.get((int(s), int(r)), [])) for s, r in zip(subs, rels)]))
    cases = topk_cases(scores.contiguous(), q_key, index, (1, 10, 100, 1000), "C2")

    rng = np.random.default_rng(0)
    Bw, n_w = 64, 123182
    wide = torch.as_tensor(rng.standard_normal((Bw, n_w)).astype(np.float32)).to(dev)
    lists = [np.unique(rng.integers(0, n_w, 20)) for _ in range(Bw)]
    keys_w = np.arange(Bw, dtype=np.int64)
    ptr_w = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    idx_w = np.concatenate(lists).astype(np.int32)
    cases += topk_cases(wide, keys_w, (keys_w, ptr_w, idx_w), (1, 10, 100, 1000), "wide123k")

    fwd, pre = summary(t["forward"]), summary(t["predict"])
    print(json.dumps(dict(probe="predict", reps=REPS, rounds=ROUNDS, C2_B=B, known_per_row=round(known_per_row, 2),
                          forward=fwd, predict=pre, predict_over_forward=round(pre["mean_ms"] / fwd["mean_ms"] - 1.0, 4),
                          topk=cases)))


if __name__ == "__main__":
    main()
