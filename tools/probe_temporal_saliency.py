"""Cost of temporal edge saliency on one explained batch: the ICEWS14-shaped synthetic of BASELINE configs[4] (C5,
synthetic.make_temporal_shape; temporal.T_RED_GNN) or synthetic.make_extrapolation_shape("X") (extrapolation.T_RED_GNN).  One JSON line:
per hop the rg_digraph_tlayer_bwd launch next to the rg_digraph_tlayer_fwd launch of the same hop inside RDigraph.saliency, that call
as a whole next to one RDigraph.rescore and next to explain, the directed source rows, the longest one and the chunk count per hop, and
how far first order carries: the facts of each row's best path deleted, estimated from the gradient (Saliency.deletion_estimate) and
re-scored exactly.  HIP events, medians (and minima) of REPEAT runs after WARMUP, all in one process.

    python tools/probe_temporal_saliency.py C5 64 [out.json]      # default out: profiles/tsaliency_C5_B64.json
    python tools/probe_temporal_saliency.py X 64 [out.json]       # default out: profiles/xsaliency_X_B64.json
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                    # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape, make_temporal_shape  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C5"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
if cfg not in ("C5", "X"):
    raise SystemExit("probe_temporal_saliency: the temporal shapes are C5 (interpolation) and X (extrapolation) (got %r)" % cfg)
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "%ssaliency_%s_B%d.json" % ("t" if cfg == "C5" else "x", cfg, B))
WARMUP, REPEAT = 3, 10
sh = SHAPES[cfg]


class P:
    pass


p = P()
p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda"
torch.manual_seed(0)
if cfg == "C5":
    from red_gnn_amd.temporal import T_RED_GNN
    kg = make_temporal_shape(cfg)
    p.n_rel, p.n_ent, p.n_time, p.graph = kg.n_rel - 1, kg.n_ent, kg.n_time, kg.quads      # the model's n_rel is the identity's id
    n_ent, n_dir, M = kg.n_ent, 3, (kg.n_rel - 1) // 2
    model = T_RED_GNN(p).cuda().eval()
    queries, objs = {"head": kg.quads[:B, 0], "relation": kg.quads[:B, 1], "time": kg.quads[:B, 3]}, None
else:
    from red_gnn_amd import extrapolation as XM
    data, n_ent, n_rel, gran = make_extrapolation_shape(cfg)
    p.n_ent, p.n_rel, p.data, p.time_granularity = n_ent, n_rel, data, gran
    n_dir, M = 1, n_rel // 2
    model = XM.T_RED_GNN(p).cuda().eval()
    late = np.flatnonzero(data[:, 3] // gran >= 200)              # full 120-day windows
    rows = data[np.sort(np.random.default_rng(5).choice(late, B, replace=False))]
    queries, objs = XM._Batch(rows[:, 0], rows[:, 1], rows[:, 3]), rows[:, 2]


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


rd, explain_ms, explain_min = timed(lambda: model.explain(queries, objs))
L = rd.n_hops
edges_h = rd.edges.cpu().numpy()
res = dict(cfg=cfg, B=B, n_dir=n_dir, n_layer=L, hidden_dim=p.hidden_dim, attn_dim=p.attn_dim, inverse_offset=M, warmup=WARMUP, repeat=REPEAT,
           chunk=engine.DIGRAPH_CHUNK, n_edges=int(edges_h.shape[0]), edges_per_hop=[int((edges_h[:, 1] == l).sum()) for l in range(1, L + 1)],
           reached=int(rd.reached.sum().item()), explain_ms=explain_ms, explain_ms_min=explain_min)
rs, res["rescore_ms"], res["rescore_ms_min"] = timed(lambda: rd.rescore(model))
sal, res["saliency_ms"], res["saliency_ms_min"] = timed(lambda: rd.saliency(model))
res["saliency_over_rescore"] = round(res["saliency_ms"] / res["rescore_ms"], 3)
res["saliency_over_explain"] = round(res["saliency_ms"] / res["explain_ms"], 3)
res["score_bits_equal_rescore"] = bool(torch.equal(sal.score, rs.score))
res["alpha_bits_equal_rescore"] = bool(torch.equal(sal.alpha, rs.alpha))
res["two_calls_bit_equal"] = bool(torch.equal(rd.saliency(model).edge_grad, sal.edge_grad))

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
    shape_bwd = [(n_rows, n_e) for (_, _, n_rows, n_e) in ev_b]
res["tlayer_fwd_ms_per_hop"] = [round(float(np.median(x)), 4) for x in fwd]
res["tlayer_bwd_ms_per_hop"] = [round(float(np.median(x)), 4) for x in bwd]
res["tlayer_fwd_ms_per_hop_min"] = [round(min(x), 4) for x in fwd]
res["tlayer_bwd_ms_per_hop_min"] = [round(min(x), 4) for x in bwd]
res["bwd_over_fwd_per_hop"] = [round(b / f, 3) for f, b in zip(res["tlayer_fwd_ms_per_hop"], res["tlayer_bwd_ms_per_hop"])]
res["bwd_over_fwd"] = round(sum(res["tlayer_bwd_ms_per_hop"]) / sum(res["tlayer_fwd_ms_per_hop"]), 3)
res["kernels_share_of_saliency"] = round((sum(res["tlayer_bwd_ms_per_hop"]) + sum(res["tlayer_fwd_ms_per_hop"])) / res["saliency_ms"], 4)
res["directed_rows_per_hop"] = [n for n, _ in shape_bwd]
# the directed source rows of every hop: out-edges per (row, head, direction)
row_q = rd.q_time.cpu().numpy().astype(np.int64)[edges_h[:, 0]]
dirn = np.sign(rd.time.cpu().numpy().astype(np.int64) - row_q) + 1 if n_dir == 3 else np.zeros(len(edges_h), np.int64)
longest, cut, chunks, used = [], [], [], []
for l in range(1, L + 1):
    at = edges_h[:, 1] == l
    e = edges_h[at]
    _, counts = np.unique((e[:, 0].astype(np.int64) * n_ent + e[:, 2]) * 3 + dirn[at], return_counts=True)
    n_hub, n_chunk, longest_l = engine.digraph_chunks(np.concatenate([[0], np.cumsum(counts)]))
    longest.append(longest_l)
    cut.append(n_hub)
    chunks.append(n_chunk)
    used.append(int(len(counts)))
res.update(longest_directed_row_per_hop=longest, cut_directed_rows_per_hop=cut, chunks_per_hop=chunks, directed_rows_with_edges_per_hop=used)

# ---- how far first order carries: the best path's facts deleted, estimated from the gradient and re-scored exactly
m = rd.top_paths(1).fact_mask(1, inverse_offset=M)
(exact, res["rescore_masked_ms"], _) = timed(lambda: rd.rescore(model, keep=~m))
est = sal.deletion_estimate(m)
ok = (exact.reached & rd.reached).cpu().numpy()
change, miss = (exact.score - rs.score).double().cpu().numpy()[ok], (est - exact.score).double().cpu().numpy()[ok]
row, fact, grad = sal.fact_grad(inverse_offset=M)
res.update(facts=int(row.numel()), rescores_one_saliency_replaces=int(row.numel()),
           one_rescore_per_fact_ms=round(float(row.numel()) * res["rescore_ms"], 1),
           best_path_rows_still_reached=int(ok.sum()), best_path_masked_edges=int(m.sum().item()),
           best_path_exact_change_mean_abs=round(float(np.abs(change).mean()), 6) if ok.any() else None,
           best_path_estimate_error_mean_abs=round(float(np.abs(miss).mean()), 6) if ok.any() else None,
           best_path_exact_change_median_abs=round(float(np.median(np.abs(change))), 6) if ok.any() else None,
           best_path_estimate_error_median_abs=round(float(np.median(np.abs(miss))), 6) if ok.any() else None,
           best_path_estimate_closer_than_no_change=round(float((np.abs(miss) < np.abs(change)).mean()), 4) if ok.any() else None,
           best_path_sign_agrees=round(float((np.sign(est.double().cpu().numpy()[ok] - rs.score.double().cpu().numpy()[ok])
                                              == np.sign(change)).mean()), 4) if ok.any() else None)
line = json.dumps(res)
print(line)
with open(out_path, "w") as fh:
    fh.write(line + "\n")
