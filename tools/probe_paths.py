"""Cost of RDigraph.top_paths on one explained batch of a BASELINE shape: one JSON line with the time of rg_paths_topk at k = 1, 4
and 8 (HIP events around engine.paths_topk: the launches of every chunk, outputs and scratch allocated), of strongest_paths() on the
same digraph (the torch route top_paths(1) replaces) and of the explain call that produced it; top_paths(1) is checked against
strongest_paths() on the way.

    python tools/probe_paths.py C2 64 [out.json]
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

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else None
WARMUP, REPEAT = 3, 10
shape = SHAPES[cfg]
kg = make_shape(cfg)
loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test), verbose=False)


class P:
    n_layer, hidden_dim, attn_dim, n_rel, act, dropout = shape["n_layer"], shape["hidden_dim"], shape["attn_dim"], kg.n_rel, "relu", 0.0


torch.manual_seed(0)
model = RED_GNN_trans(P, loader).cuda().eval()
model.use_graphs = False                       # the eager forward is what explain runs
q = np.arange(B) % loader.n_test
subs = np.array([loader.test_q[i][0] for i in q])
rels = np.array([loader.test_q[i][1] for i in q])


def timed(f):
    """(last result, median and minimum ms over REPEAT runs after WARMUP, by device events)."""
    ms = []
    for i in range(WARMUP + REPEAT):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = f()
        t.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(s.elapsed_time(t))
    return out, round(float(np.median(ms)), 4), round(min(ms), 4)


rd, explain_ms, explain_min = timed(lambda: model.explain(subs, rels))
L = rd.n_hops
off = rd.offsets.cpu().numpy()
edges_h = rd.edges.cpu().numpy()
res = dict(cfg=cfg, B=B, n_layer=L, warmup=WARMUP, repeat=REPEAT, n_edges=int(off[-1]), edges_per_row_max=int(np.diff(off).max()),
           edges_per_hop=[int((edges_h[:, 1] == l).sum()) for l in range(1, L + 1)],
           groups_per_hop=[int(len(np.unique(edges_h[edges_h[:, 1] == l][:, [0, 4]], axis=0))) for l in range(1, L + 1)],
           reached=int(rd.reached.sum().item()), explain_ms=explain_ms, explain_ms_min=explain_min)
(r1, e1, p1), res["strongest_paths_ms"], res["strongest_paths_ms_min"] = timed(rd.strongest_paths)
for k in (1, 4, 8):
    res["scratch_bytes_k%d" % k] = engine.paths_scratch_bytes(int(off[-1]), k)
    got, res["paths_topk_k%d_ms" % k], res["paths_topk_k%d_ms_min" % k] = timed(
        lambda: engine.paths_topk(rd.edges, rd.alpha, rd.offsets, L, k, offsets_host=off))
    res["paths_k%d" % k] = int(got[2].sum().item())
ps = rd.top_paths(1)
res["k1_equals_strongest_paths"] = bool(torch.equal(ps.rels()[:, 0], r1) and torch.equal(ps.entities()[:, 0], e1)
                                        and torch.equal(ps.product[:, 0], p1))
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as f:
        f.write(line + "\n")
