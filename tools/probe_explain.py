"""Cost of RED_GNN_trans.explain on a BASELINE shape: one JSON line with the eager forward's time, explain's total time and its HIP
kernels' time per hop (HIP events around rg_explain_count + rg_explain_emit), marked-tail words and emitted edges per hop against the
subgraph's edges per hop, and the marking pass's bytes by DESIGN.md §4's model.

    python tools/probe_explain.py C2 1024
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.load_data import DataLoader                      # noqa: E402
from red_gnn_amd.models import RED_GNN_trans                      # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_shape              # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
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
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


with torch.no_grad():
    for _ in range(2):
        _, t_fwd = timed(lambda: model(subs, rels, mode="test"))
    sub_edges = list(model.last_stats["n_edges"])
    for _ in range(2):
        ev = engine.EXPLAIN_EVENTS = []
        rd, t_exp = timed(lambda: model.explain(subs, rels))
    engine.EXPLAIN_EVENTS = None
L = shape["n_layer"]
e = rd.edges.cpu().numpy()
per_hop_ms = {int(lvl): s.elapsed_time(t) for (s, t, lvl, _) in ev}
emitted = [int((e[:, 1] == l).sum()) for l in range(1, L + 1)]
marked_tails = [int(len(np.unique(e[e[:, 1] == l][:, [0, 4]], axis=0))) for l in range(1, L + 1)]
# DESIGN.md §4 byte model of one hop's marking pass (count + emit read the same data): the mark words (4 B per (row, entity word)),
# per marked tail its CSR row (8 B per in-edge + 8 B of in_ptr) and per in-edge the level word of its head (8 B); where the head is in
# the level (= the emitted edges at min_alpha 0) its a_s row and the relation's a_r row (4 * ap B each); emit adds 20 B written per edge
ap = 4 * ((shape["attn_dim"] + 3) // 4)
g = loader.tgraph
_, _, ip, _ = g.export()
indeg = np.diff(ip)
W = (kg.n_ent + 31) // 32
hop_bytes, cands = [], []
for l in range(1, L + 1):
    tails = e[e[:, 1] == l][:, [0, 4]]
    tails = np.unique(tails, axis=0)
    cand = int(indeg[tails[:, 1]].sum()) if len(tails) else 0
    cands.append(cand)
    rd_bytes = 4 * B * W + 8 * len(tails) + 16 * cand + 8 * ap * emitted[l - 1]
    hop_bytes.append(2 * rd_bytes + 20 * emitted[l - 1])
print(json.dumps(dict(cfg=cfg, B=B, n_layer=L, forward_ms=round(t_fwd, 3), explain_ms=round(t_exp, 3),
                      explain_kernel_ms_per_hop={l: round(per_hop_ms.get(l, 0.0), 3) for l in range(1, L + 1)},
                      explain_kernel_ms=round(sum(per_hop_ms.values()), 3), marked_tails_per_hop=marked_tails,
                      emitted_edges_per_hop=emitted, candidate_in_edges_per_hop=cands, subgraph_edges_per_hop=sub_edges, model_bytes_per_hop=hop_bytes,
                      reached=int(rd.reached.sum().item()))))
