"""Cost and additivity of integrated gradients on one explained batch of a BASELINE shape (tools/probe_saliency.py's batch): one JSON
line with RDigraph.integrated_gradients(steps=16) next to one RDigraph.saliency and next to 16 sequential saliency(gate=...) calls at
the same midpoints; the gated, replicated edge-list kernels per hop (16 replicas in one launch) next to the ungated ones (one
replica); the residual per row at 4 / 16 / 64 steps; and, for the facts of each row's best path, the sum of their fact_attr next to
the exact rescore change and next to Saliency.deletion_estimate.  HIP events, medians (and minima) of REPEAT runs after WARMUP, one
process.

    python tools/probe_ig.py C2 64 [out.json]        (default: profiles/ig_<cfg>_B<batch>.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.load_data import DataLoader                      # noqa: E402
from red_gnn_amd.models import RED_GNN_trans                      # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_shape              # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "ig_%s_B%d.json" % (cfg, B))
WARMUP, REPEAT, STEPS = 3, 10, 16
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


rd = model.explain(subs, rels)
L, E = rd.n_hops, rd.edges.shape[0]
edges_h = rd.edges.cpu().numpy()
res = dict(cfg=cfg, B=B, n_layer=L, hidden_dim=P.hidden_dim, attn_dim=P.attn_dim, warmup=WARMUP, repeat=REPEAT, steps=STEPS,
           n_edges=int(E), edges_per_hop=[int((edges_h[:, 1] == l).sum()) for l in range(1, L + 1)], reached=int(rd.reached.sum().item()))
rs, res["rescore_ms"], res["rescore_ms_min"] = timed(lambda: rd.rescore(model))
sal, res["saliency_ms"], res["saliency_ms_min"] = timed(lambda: rd.saliency(model))
att, res["ig_ms"], res["ig_ms_min"] = timed(lambda: rd.integrated_gradients(model, steps=STEPS))

# ---- the same quadrature as STEPS sequential saliencies at the midpoints' gates: what the replicas save
lo = (rd.edges[:, 3] == 2 * model.n_rel).float()
mids = [(lo + ((k + 0.5) / STEPS) * (1.0 - lo)).contiguous() for k in range(STEPS)]


def sequential():
    acc = torch.zeros(E, device="cuda")
    for g in mids:
        acc += (1.0 - lo) / STEPS * rd.saliency(model, gate=g).edge_grad
    return acc


seq, res["sequential_ms"], res["sequential_ms_min"] = timed(sequential)
res["sequential_max_abs_diff"] = float((seq - att.edge_attr).abs().max())
res["ig_over_saliency"] = round(res["ig_ms"] / res["saliency_ms"], 3)
res["sequential_over_ig"] = round(res["sequential_ms"] / res["ig_ms"], 3)
res["rep_chunk_3_ms"], res["rep_chunk_3_ms_min"] = timed(lambda: rd.integrated_gradients(model, steps=STEPS, rep_chunk=3))[1:]


# ---- the edge-list kernels per hop: gated with STEPS replicas (inside integrated_gradients) next to ungated (inside saliency)
def kernel_events(f, n_fwd_skip):
    fwd, bwd = [[] for _ in range(L)], [[] for _ in range(L)]
    for i in range(WARMUP + REPEAT):
        engine.DIGRAPH_EVENTS, engine.DIGRAPH_BWD_EVENTS = [], []
        f()
        torch.cuda.synchronize()
        ev_f, ev_b = engine.DIGRAPH_EVENTS[n_fwd_skip:], engine.DIGRAPH_BWD_EVENTS[::-1]   # the backward walks the hops from L down to 1
        engine.DIGRAPH_EVENTS = engine.DIGRAPH_BWD_EVENTS = None
        if i >= WARMUP:
            for l in range(L):
                fwd[l].append(ev_f[l][0].elapsed_time(ev_f[l][1]))
                bwd[l].append(ev_b[l][0].elapsed_time(ev_b[l][1]))
    med = lambda xs: [round(float(np.median(x)), 4) for x in xs]
    return med(fwd), med(bwd), [round(min(x), 4) for x in fwd], [round(min(x), 4) for x in bwd]


res["layer_fwd_ms_per_hop"], res["layer_bwd_ms_per_hop"], res["layer_fwd_ms_per_hop_min"], res["layer_bwd_ms_per_hop_min"] = \
    kernel_events(lambda: rd.saliency(model), 0)
# (integrated_gradients first runs the two ends of the path, L forward launches of two replicas, then one group of STEPS replicas)
res["gated_fwd_ms_per_hop"], res["gated_bwd_ms_per_hop"], res["gated_fwd_ms_per_hop_min"], res["gated_bwd_ms_per_hop_min"] = \
    kernel_events(lambda: rd.integrated_gradients(model, steps=STEPS), L)
res["gated_fwd_ms_per_hop_1rep"], res["gated_bwd_ms_per_hop_1rep"] = kernel_events(lambda: rd.saliency(model, gate=mids[0]), 0)[:2]
res["gated_over_ungated_per_replica"] = round((sum(res["gated_fwd_ms_per_hop"]) + sum(res["gated_bwd_ms_per_hop"])) / STEPS /
                                              (sum(res["layer_fwd_ms_per_hop"]) + sum(res["layer_bwd_ms_per_hop"])), 4)

# ---- the residual per row: what the midpoint rule leaves of score - baseline_score
for steps in (4, 16, 64):
    a = att if steps == STEPS else rd.integrated_gradients(model, steps=steps)
    r = a.residual.double().abs().cpu().numpy()
    res["residual_abs_steps_%d" % steps] = dict(mean=round(float(r.mean()), 7), median=round(float(np.median(r)), 7), max=round(float(r.max()), 7))
res["score_minus_baseline_abs_mean"] = round(float((att.score - att.baseline_score).double().abs().mean()), 6)
res["score_bits_equal_rescore"] = bool(torch.equal(att.score, rs.score))

# ---- the best path's facts: their attributions summed, the exact rescore change, and the tangent's estimate
m = rd.top_paths(1).fact_mask(1)
exact = rd.rescore(model, keep=~m)
est = sal.deletion_estimate(m)
ok = (exact.reached & rd.reached).cpu().numpy()
row = rd.edges[:, 0].long()
attr_sum = torch.zeros(B, device="cuda", dtype=torch.float64).index_add(0, row[m], att.edge_attr[m].double()).cpu().numpy()[ok]
change = (rs.score - exact.score).double().cpu().numpy()[ok]                  # what the answer loses when the facts go
tangent = (rs.score - est).double().cpu().numpy()[ok]                         # ... by the gradient at gate 1
res.update(best_path_rows_still_reached=int(ok.sum()), best_path_masked_edges=int(m.sum().item()),
           best_path_exact_change_mean_abs=round(float(np.abs(change).mean()), 6),
           best_path_attr_sum_mean_abs=round(float(np.abs(attr_sum).mean()), 6),
           best_path_attr_minus_change_mean_abs=round(float(np.abs(attr_sum - change).mean()), 6),
           best_path_attr_minus_change_median_abs=round(float(np.median(np.abs(attr_sum - change))), 6),
           best_path_tangent_minus_change_mean_abs=round(float(np.abs(tangent - change).mean()), 6),
           best_path_tangent_minus_change_median_abs=round(float(np.median(np.abs(tangent - change))), 6),
           best_path_attr_closer_than_tangent=round(float((np.abs(attr_sum - change) < np.abs(tangent - change)).mean()), 4),
           best_path_attr_sign_agrees=round(float((np.sign(attr_sum) == np.sign(change)).mean()), 4))
line = json.dumps(res)
print(line)
with open(out_path, "w") as fh:
    fh.write(line + "\n")
