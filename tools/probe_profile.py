"""Cost of RED_GNN_trans.attention_profile on a BASELINE shape: one JSON line with, per hop, the time of the profile kernel
(HIP events around rg_attn_profile) next to the time of the forward's walk (rg_layer_fwd) for the same batch in the same process, the
edges per hop, and the profile pass's bytes by DESIGN.md §4's model.

    python tools/probe_profile.py C2 1024
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
q = np.arange(B) % loader.n_test
subs = np.array([loader.test_q[i][0] for i in q])
rels = np.array([loader.test_q[i][1] for i in q])
L = shape["n_layer"]


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


REPS = 3
with torch.no_grad():
    walk_ms, prof_ms = [], []
    for _ in range(1 + REPS):                  # the first round warms up
        trace = []
        fev = engine.KERNEL_EVENTS = []        # (collecting events keeps the forward eager: the path attention_profile runs)
        _, t_fwd = timed(lambda: model(subs, rels, mode="test", trace=trace))
        engine.KERNEL_EVENTS = None
        sub_edges = list(model.last_stats["n_edges"])
        walk_ms.append([s.elapsed_time(t) for (s, t, _, _) in fev])
        pev = engine.PROFILE_EVENTS = []
        prof, t_prof = timed(lambda: model.attention_profile(subs, rels))
        engine.PROFILE_EVENTS = None
        by_level = {lvl: s.elapsed_time(t) for (s, t, lvl) in pev}
        prof_ms.append([by_level[l] for l in range(1, L + 1)])
walk_ms, prof_ms = np.array(walk_ms[1:]), np.array(prof_ms[1:])
assert prof.count.sum((0, 2)).tolist() == sub_edges
# DESIGN.md §4 byte model of one hop of the profile pass: the level-(l-1) words of every query (8 B per (query, entity word)), per
# head of that level its out_ptr pair (8 B) and its a_s row (4 * ap B), per edge its CSR-by-head entry (8 B); a_r and the bins stay
# in LDS.  Every out-edge of a level-(l-1) node is an edge of the hop: nothing is read in vain.
ap = 4 * ((shape["attn_dim"] + 3) // 4)
W = (kg.n_ent + 31) // 32
heads = [B] + [int(trace[l]["nodes"].shape[0]) for l in range(L - 1)]
hop_bytes = [8 * B * W + (8 + 4 * ap) * heads[l] + 8 * sub_edges[l] for l in range(L)]
r3 = lambda a: [round(float(x), 3) for x in a]
print(json.dumps(dict(cfg=cfg, B=B, n_layer=L, reps=REPS, forward_ms=round(t_fwd, 3), attention_profile_ms=round(t_prof, 3),
                      profile_kernel_ms_per_hop=r3(np.median(prof_ms, 0)), profile_kernel_ms_per_hop_min=r3(prof_ms.min(0)),
                      profile_kernel_ms_per_hop_max=r3(prof_ms.max(0)),
                      forward_walk_ms_per_hop=r3(np.median(walk_ms, 0)), forward_walk_ms_per_hop_min=r3(walk_ms.min(0)),
                      forward_walk_ms_per_hop_max=r3(walk_ms.max(0)),
                      edges_per_hop=sub_edges, heads_per_hop=heads, model_bytes_per_hop=hop_bytes,
                      model_gbytes_per_s_per_hop=r3(np.array(hop_bytes) / (np.median(prof_ms, 0) * 1e6)))))
