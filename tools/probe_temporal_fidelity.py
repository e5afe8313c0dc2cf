"""Cost of temporal explanation fidelity on one explained batch of the ICEWS14-shaped synthetic of BASELINE configs[4] (C5,
synthetic.make_temporal_shape): one JSON line with the time of the temporal RDigraph.rescore(keep=None) as a whole and of its
rg_digraph_tlayer_fwd launch per hop, of the 2k rescores of T_RED_GNN.fidelity (the quadruples of the best j paths deleted / kept
alone, j = 1..k) and of the fidelity call itself, next to T_RED_GNN.explain on the same batch and RDigraph.top_paths(k), all in one
process and one window; edges per hop, the longest destination list and the chunk count per hop go with them.  HIP events, medians
(and minima) of REPEAT runs after WARMUP.  tools/probe_fidelity.py is the static model's.

    python tools/probe_temporal_fidelity.py C5 64 [out.json]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_temporal_shape     # noqa: E402
from red_gnn_amd.temporal import T_RED_GNN                        # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C5"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else None
if cfg != "C5":
    raise SystemExit("probe_temporal_fidelity: the temporal shape is C5 (got %r)" % cfg)
K = 4
WARMUP, REPEAT = 3, 10
sh = SHAPES[cfg]
kg = make_temporal_shape(cfg)
quads = kg.quads


class P:
    pass


p = P()
# the model's n_rel is the identity's relation id (kg.n_rel counts it): fidelity keeps the edges of relation model.n_rel as self-loops
p.n_rel, p.n_ent, p.n_time, p.graph = kg.n_rel - 1, kg.n_ent, kg.n_time, kg.quads
p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda"
M = (kg.n_rel - 1) // 2                        # the inverse of base relation r is r + M
torch.manual_seed(0)
model = T_RED_GNN(p).cuda().eval()
batch = {"head": quads[:B, 0], "relation": quads[:B, 1], "time": quads[:B, 3]}


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


rd, explain_ms, explain_min = timed(lambda: model.explain(batch))
L = rd.n_hops
edges_h = rd.edges.cpu().numpy()
res = dict(cfg=cfg, B=B, k=K, n_layer=L, hidden_dim=p.hidden_dim, attn_dim=p.attn_dim, inverse_offset=M, warmup=WARMUP, repeat=REPEAT,
           chunk=engine.DIGRAPH_CHUNK, n_edges=int(edges_h.shape[0]), edges_per_hop=[int((edges_h[:, 1] == l).sum()) for l in range(1, L + 1)],
           reached=int(rd.reached.sum().item()), explain_ms=explain_ms, explain_ms_min=explain_min)
paths, res["top_paths_ms"], res["top_paths_ms_min"] = timed(lambda: rd.top_paths(K))

# ---- rescore(keep=None): the whole call, and the message-passing launch of every hop
rs, res["rescore_all_ms"], res["rescore_all_ms_min"] = timed(lambda: rd.rescore(model))
res["rescore_all_max_abs_diff_to_score"] = float((rs.score - rd.score).abs().max().item())
# (a random-init relu model of five layers scores in the 1e9s on this shape: the relative figure is the one to read)
res["score_abs_max"] = float(rd.score.abs().max().item())
res["rescore_all_max_rel_diff_to_score"] = float(((rs.score - rd.score).abs() / rd.score.abs().clamp(min=1.0)).max().item())
per_hop = [[] for _ in range(L)]
shape_per_hop = None
for i in range(WARMUP + REPEAT):
    engine.DIGRAPH_EVENTS = []
    rd.rescore(model)
    torch.cuda.synchronize()
    ev, engine.DIGRAPH_EVENTS = engine.DIGRAPH_EVENTS, None
    if i >= WARMUP:
        for l, (s, t, n_dst, n_e) in enumerate(ev):
            per_hop[l].append(s.elapsed_time(t))
    shape_per_hop = [(n_dst, n_e) for (_, _, n_dst, n_e) in ev]
res["tlayer_ms_per_hop"] = [round(float(np.median(x)), 4) for x in per_hop]
res["tlayer_ms_per_hop_min"] = [round(min(x), 4) for x in per_hop]
res["destinations_per_hop"] = [n for n, _ in shape_per_hop]
longest, cut, chunks = [], [], []
for l in range(1, L + 1):
    e = edges_h[edges_h[:, 1] == l]
    _, counts = np.unique(e[:, 0].astype(np.int64) * kg.n_ent + e[:, 4], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    n_hub, n_chunk, longest_l = engine.digraph_chunks(ptr)
    longest.append(longest_l)
    cut.append(n_hub)
    chunks.append(n_chunk)
res.update(longest_destination_per_hop=longest, cut_destinations_per_hop=cut, chunks_per_hop=chunks)

# ---- the 2k rescores of fidelity, each alone, then the call as a whole (explain + top_paths + 2k rescores + the masks)
loops = rd.edges[:, 3] == model.n_rel
res["self_loop_edges"] = int(loops.sum().item())
without_ms, only_ms, live_without, live_only = [], [], [], []
for j in range(1, K + 1):
    m = paths.fact_mask(j, inverse_offset=M)
    keep_wo, keep_on = ~m, m | loops
    r, ms, _ = timed(lambda: rd.rescore(model, keep=keep_wo))
    without_ms.append(ms)
    live_without.append(int(r.live.sum().item()))
    r, ms, _ = timed(lambda: rd.rescore(model, keep=keep_on))
    only_ms.append(ms)
    live_only.append(int(r.live.sum().item()))
res.update(rescore_without_ms=without_ms, rescore_only_ms=only_ms, live_edges_without=live_without, live_edges_only=live_only)
_, res["fact_mask_ms"], res["fact_mask_ms_min"] = timed(lambda: paths.fact_mask(K, inverse_offset=M))
f, res["fidelity_ms"], res["fidelity_ms_min"] = timed(lambda: model.fidelity(batch, k=K, inverse_offset=M))
res["necessity_mean"] = [round(v, 6) for v in f.necessity().double().mean(0).tolist()]
res["sufficiency_gap_mean"] = [round(v, 6) for v in f.sufficiency_gap().double().mean(0).tolist()]
res["disconnected"] = (rd.reached[:, None] & ~f.reached_without).double().mean(0).tolist()
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
