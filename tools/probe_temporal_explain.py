"""Cost of T_RED_GNN.attention_profile and T_RED_GNN.explain on the ICEWS14-shaped synthetic of BASELINE configs[4] (C5,
synthetic.make_temporal_shape): one JSON line with, per hop, the time of the profile kernel (HIP events around rg_tattn_profile), of the
count + emit pair of the r-digraph extraction (rg_texplain_count + rg_texplain_emit, explaining every query's top answer) and of the
forward's layer kernel (rg_tlayer_fwd) for the same batch in the same process.

    python tools/probe_temporal_explain.py C5 64 > profiles/tattn_profile_C5_B64.json
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_temporal_shape     # noqa: E402
from red_gnn_amd.temporal import T_RED_GNN                        # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C5"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
if cfg != "C5":
    raise SystemExit("probe_temporal_explain: the temporal shape is C5 (got %r)" % cfg)
sh = SHAPES[cfg]
kg = make_temporal_shape(cfg)
quads = kg.quads


class P:
    pass


p = P()
p.n_rel, p.n_ent, p.n_time, p.graph = kg.n_rel, kg.n_ent, kg.n_time, kg.quads
p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda"
n_rel = kg.n_rel
torch.manual_seed(0)
model = T_RED_GNN(p).cuda().eval()
batch = {"head": quads[:B, 0], "relation": quads[:B, 1], "time": quads[:B, 3]}
L = sh["n_layer"]


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


REPS = 3
with torch.no_grad():
    layer_ms, prof_ms, expl_ms, expl_edges = [], [], [], []
    for _ in range(1 + REPS):                  # the first round warms up
        fev = engine.KERNEL_EVENTS = []
        _, t_fwd = timed(lambda: model(batch, mode="test"))
        engine.KERNEL_EVENTS = None
        sub_edges = list(model.last_stats["n_edges"])
        layer_ms.append([s.elapsed_time(e) for (s, e, _, _) in fev])
        pev = engine.PROFILE_EVENTS = []
        prof, t_prof = timed(lambda: model.attention_profile(batch))
        engine.PROFILE_EVENTS = None
        by_level = {lvl: s.elapsed_time(e) for (s, e, lvl) in pev}
        prof_ms.append([by_level[l] for l in range(1, L + 1)])
        xev = engine.EXPLAIN_EVENTS = []
        rd, t_expl = timed(lambda: model.explain(batch))
        engine.EXPLAIN_EVENTS = None
        by_level = {lvl: (s.elapsed_time(e), n) for (s, e, lvl, n) in xev}
        expl_ms.append([by_level[l][0] for l in range(1, L + 1)])
        expl_edges = [by_level[l][1] for l in range(1, L + 1)]
layer_ms, prof_ms, expl_ms = np.array(layer_ms[1:]), np.array(prof_ms[1:]), np.array(expl_ms[1:])
assert prof.count.sum((0, 2, 3)).tolist() == sub_edges
r3 = lambda a: [round(float(x), 3) for x in a]
print(json.dumps(dict(cfg=cfg, B=B, n_layer=L, reps=REPS, n_rela_rows=n_rel + 1, attn_dim=sh["attn_dim"], hidden_dim=sh["hidden_dim"],
                      forward_ms=round(t_fwd, 3), attention_profile_ms=round(t_prof, 3), explain_ms=round(t_expl, 3),
                      edges_per_hop=sub_edges, digraph_edges_per_hop=expl_edges,
                      profile_kernel_ms_per_hop=r3(np.median(prof_ms, 0)), profile_kernel_ms_per_hop_min=r3(prof_ms.min(0)),
                      profile_kernel_ms_per_hop_max=r3(prof_ms.max(0)),
                      explain_pair_ms_per_hop=r3(np.median(expl_ms, 0)), explain_pair_ms_per_hop_min=r3(expl_ms.min(0)),
                      explain_pair_ms_per_hop_max=r3(expl_ms.max(0)),
                      forward_layer_ms_per_hop=r3(np.median(layer_ms, 0)), forward_layer_ms_per_hop_min=r3(layer_ms.min(0)),
                      forward_layer_ms_per_hop_max=r3(layer_ms.max(0)),
                      profile_over_layer_per_hop=r3(np.median(prof_ms, 0) / np.median(layer_ms, 0)))))
