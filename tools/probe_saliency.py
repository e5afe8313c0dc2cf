"""Cost of edge saliency on one explained batch of a BASELINE shape: one JSON line with, per hop, the time of rg_digraph_layer_bwd next
to rg_digraph_layer_fwd on the same hop (both inside RDigraph.saliency), the whole saliency call next to one RDigraph.rescore and next
to the explain call of the same batch, and - for the facts of each row's best path - Saliency.deletion_estimate next to the exact
rescore, so that one sees how far first order carries.  Sources per hop, the longest out-list and the chunk count per hop go with
them.  HIP events, medians (and minima) of REPEAT runs after WARMUP, one process.

    python tools/probe_saliency.py C2 64 [out.json]
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
edges_h = rd.edges.cpu().numpy()
res = dict(cfg=cfg, B=B, n_layer=L, hidden_dim=P.hidden_dim, attn_dim=P.attn_dim, warmup=WARMUP, repeat=REPEAT,
           chunk=engine.DIGRAPH_CHUNK, n_edges=int(edges_h.shape[0]), edges_per_hop=[int((edges_h[:, 1] == l).sum()) for l in range(1, L + 1)],
           reached=int(rd.reached.sum().item()), explain_ms=explain_ms, explain_ms_min=explain_min)
rs, res["rescore_ms"], res["rescore_ms_min"] = timed(lambda: rd.rescore(model))
sal, res["saliency_ms"], res["saliency_ms_min"] = timed(lambda: rd.saliency(model))
res["saliency_over_rescore"] = round(res["saliency_ms"] / res["rescore_ms"], 3)
res["saliency_over_explain"] = round(res["saliency_ms"] / res["explain_ms"], 3)
res["score_bits_equal_rescore"] = bool(torch.equal(sal.score, rs.score))

# ---- the two edge-list kernels of every hop inside saliency: the forward launch, and the backward launch of the same hop
fwd, bwd = [[] for _ in range(L)], [[] for _ in range(L)]
shape_bwd = None
for i in range(WARMUP + REPEAT):
    engine.DIGRAPH_EVENTS, engine.DIGRAPH_BWD_EVENTS = [], []
    rd.saliency(model)
    torch.cuda.synchronize()
    ev_f, ev_b = engine.DIGRAPH_EVENTS, engine.DIGRAPH_BWD_EVENTS[::-1]          # the backward walks the hops from L down to 1
    engine.DIGRAPH_EVENTS = engine.DIGRAPH_BWD_EVENTS = None
    if i >= WARMUP:
        for l in range(L):
            fwd[l].append(ev_f[l][0].elapsed_time(ev_f[l][1]))
            bwd[l].append(ev_b[l][0].elapsed_time(ev_b[l][1]))
    shape_bwd = [(n_src, n_e) for (_, _, n_src, n_e) in ev_b]
res["layer_fwd_ms_per_hop"] = [round(float(np.median(x)), 4) for x in fwd]
res["layer_bwd_ms_per_hop"] = [round(float(np.median(x)), 4) for x in bwd]
res["layer_fwd_ms_per_hop_min"] = [round(min(x), 4) for x in fwd]
res["layer_bwd_ms_per_hop_min"] = [round(min(x), 4) for x in bwd]
res["bwd_over_fwd_per_hop"] = [round(b / f, 3) for f, b in zip(res["layer_fwd_ms_per_hop"], res["layer_bwd_ms_per_hop"])]
res["bwd_over_fwd"] = round(sum(res["layer_bwd_ms_per_hop"]) / sum(res["layer_fwd_ms_per_hop"]), 3)
res["sources_per_hop"] = [n for n, _ in shape_bwd]
longest, cut, chunks = [], [], []
for l in range(1, L + 1):
    e = edges_h[edges_h[:, 1] == l]
    _, counts = np.unique(e[:, 0].astype(np.int64) * loader.n_ent + e[:, 2], return_counts=True)        # out-edges per (row, head)
    n_hub, n_chunk, longest_l = engine.digraph_chunks(np.concatenate([[0], np.cumsum(counts)]))
    longest.append(longest_l)
    cut.append(n_hub)
    chunks.append(n_chunk)
res.update(longest_source_per_hop=longest, cut_sources_per_hop=cut, chunks_per_hop=chunks)

# ---- how far first order carries: the best path's facts deleted, estimated from the gradient and re-scored exactly
m = rd.top_paths(1).fact_mask(1)
exact = rd.rescore(model, keep=~m)
est = sal.deletion_estimate(m)
ok = (exact.reached & rd.reached).cpu().numpy()
change, miss = (exact.score - rs.score).double().cpu().numpy()[ok], (est - exact.score).double().cpu().numpy()[ok]
res.update(best_path_rows_still_reached=int(ok.sum()), best_path_masked_edges=int(m.sum().item()),
           best_path_exact_change_mean_abs=round(float(np.abs(change).mean()), 6), best_path_estimate_error_mean_abs=round(float(np.abs(miss).mean()), 6),
           best_path_exact_change_median_abs=round(float(np.median(np.abs(change))), 6),
           best_path_estimate_error_median_abs=round(float(np.median(np.abs(miss))), 6),
           best_path_estimate_closer_than_no_change=round(float((np.abs(miss) < np.abs(change)).mean()), 4),
           best_path_sign_agrees=round(float((np.sign(est.double().cpu().numpy()[ok] - rs.score.double().cpu().numpy()[ok]) == np.sign(change)).mean()), 4))
line = json.dumps(res)
print(line)
if out_path:
    with open(out_path, "w") as fh:
        fh.write(line + "\n")
