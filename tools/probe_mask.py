"""Cost and outcome of learned edge masks on one explained batch of a BASELINE shape (tools/probe_saliency.py's batch): one JSON
line with, per iteration of RDigraph.learn_mask, the three launches (the gated forward, the gated adjoint, rg_mask_step) next to the
torch glue around them; rg_mask_step next to the same update written in torch (what the fusing saves - a measurement, not a target);
R replicas in one walk next to R one-replica walks; per lambda the mean size / n_free and |kept_score - target| / scale of its own
mask; and EdgeMask.keep next to top_paths(4).fact_mask in size and sufficiency gap.  HIP events, medians (and minima) of REPEAT runs
after WARMUP, one process.

    python tools/probe_mask.py C2 64 [out.json]        (default: profiles/mask_<cfg>_B<batch>.json)
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine, explain                          # noqa: E402
from red_gnn_amd.load_data import DataLoader                      # noqa: E402
from red_gnn_amd.models import RED_GNN_trans                      # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_shape              # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "mask_%s_B%d.json" % (cfg, B))
WARMUP, REPEAT, ITERATIONS = 2, 5, 100
LAMBDAS = (0.01, 0.03, 0.1, 0.3, 1.0)                            # learn_mask's defaults
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


def timed(f, repeat=REPEAT):
    """(last result, median and minimum ms over ``repeat`` runs after WARMUP, by device events)."""
    ms = []
    for i in range(WARMUP + repeat):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = f()
        t.record()
        torch.cuda.synchronize()
        if i >= WARMUP:
            ms.append(s.elapsed_time(t))
    return out, round(float(np.median(ms)), 4), round(min(ms), 4)


rd = model.explain(subs, rels)
L, E, R = rd.n_hops, rd.edges.shape[0], len(LAMBDAS)
res = dict(cfg=cfg, B=B, n_layer=L, hidden_dim=P.hidden_dim, attn_dim=P.attn_dim, warmup=WARMUP, repeat=REPEAT, iterations=ITERATIONS,
           lambdas=list(LAMBDAS), n_edges=int(E), reached=int(rd.reached.sum().item()))
res["saliency_ms"] = timed(lambda: rd.saliency(model))[1]
short, res["learn_mask_10_iterations_ms"], _ = timed(lambda: rd.learn_mask(model, iterations=10))
_, res["learn_mask_0_iterations_ms"], _ = timed(lambda: rd.learn_mask(model, iterations=0))
res["ms_per_iteration"] = round((res["learn_mask_10_iterations_ms"] - res["learn_mask_0_iterations_ms"]) / 10, 4)

# ---- one iteration taken apart: the walk (forward + adjoint, their HIP launches by their own events) and the step
S, _ = explain._gated_setup(rd, model, None, "test", "probe", {})
hops, live, reached = explain._static_hops(S, "probe")
gate = short.replica_gate.clone()


def walk(g, split_dense=True):
    return explain._gated_group(S, rd, model, hops, None, None, None, True, check_index=False, gate=g, split_dense=split_dense)


# (learn_mask runs the dense adjoint per replica, which is what makes a replica's gradient the one-replica call's bit for bit; the
# stacked adjoint is what integrated gradients runs)
(score, _, grad), res["walk_ms"], res["walk_ms_min"] = timed(lambda: walk(gate))
(_, _, grad_st), res["walk_stacked_dense_adjoint_ms"], _ = timed(lambda: walk(gate, False))
res["stacked_dense_adjoint_max_abs_grad_diff"] = float((grad - grad_st).abs().max())
fwd_ms, bwd_ms = [], []
for i in range(WARMUP + REPEAT):
    engine.DIGRAPH_EVENTS, engine.DIGRAPH_BWD_EVENTS = [], []
    walk(gate)
    torch.cuda.synchronize()
    ev_f, ev_b = engine.DIGRAPH_EVENTS, engine.DIGRAPH_BWD_EVENTS
    engine.DIGRAPH_EVENTS = engine.DIGRAPH_BWD_EVENTS = None
    if i >= WARMUP:
        fwd_ms.append(sum(a.elapsed_time(b) for a, b, _, _ in ev_f))
        bwd_ms.append(sum(a.elapsed_time(b) for a, b, _, _ in ev_b))
res["gates_fwd_launches_ms"], res["gates_bwd_launches_ms"] = round(float(np.median(fwd_ms)), 4), round(float(np.median(bwd_ms)), 4)

free = (rd.edges[:, 3] != 2 * model.n_rel)
free_u8 = free.to(torch.uint8)
row = rd.edges[:, 0].long()
scale = (short.target - short.baseline_score).abs()
inv_scale = torch.where((scale > 0) & short.reached, 1.0 / scale, torch.zeros_like(scale))
inv_n = torch.where(short.n_free > 0, 1.0 / short.n_free.float(), torch.zeros(B, device="cuda"))
lam_s, lam_e = torch.tensor(LAMBDAS, device="cuda"), torch.zeros(R, device="cuda")
state = [torch.full((R, E), 2.0, device="cuda"), torch.zeros((R, E), device="cuda"), torch.zeros((R, E), device="cuda")]


def hip_step():
    th, m, v = (x.clone() for x in state)
    return engine.mask_step(rd.offsets, free_u8, score, short.target, inv_scale, inv_n, lam_s, lam_e, grad, th, m, v, 3, gate_out=gate.clone())


def torch_step(b1=0.9, b2=0.999, eps=1e-8, lr=0.05, t=3):
    th, m, v = (x.clone() for x in state)
    g = torch.sigmoid(th)
    coef = 2 * (score - short.target[None]) * inv_scale[None] ** 2
    dl = coef[:, row] * grad + (lam_s[:, None] * inv_n[None])[:, row] - lam_e[:, None] * th
    gt = dl * g * (1 - g)
    m1, v1 = b1 * m + (1 - b1) * gt, b2 * v + (1 - b2) * gt * gt
    th1 = th - lr * (m1 / (1 - b1 ** t)) / ((v1 / (1 - b2 ** t)).sqrt() + eps)
    th, m, v = torch.where(free[None], th1, th), torch.where(free[None], m1, m), torch.where(free[None], v1, v)
    g1 = torch.where(free[None], torch.sigmoid(th), gate)
    gf = torch.where(free[None], g1, torch.zeros_like(g1))
    size = torch.zeros((R, B), device="cuda").index_add_(1, row, gf)
    count = torch.zeros((R, B), device="cuda", dtype=torch.int64).index_add_(1, row, (gf > 0.5).long())
    return g1, size, count


a, res["mask_step_ms"], res["mask_step_ms_min"] = timed(hip_step, 20)
b, res["torch_step_ms"], res["torch_step_ms_min"] = timed(torch_step, 20)
res["mask_step_vs_torch_max_abs_gate_diff"] = float((a[0] - b[0]).abs().max())
res["torch_over_mask_step"] = round(res["torch_step_ms"] / res["mask_step_ms"], 2)
res["glue_ms_per_iteration"] = round(res["walk_ms"] - res["gates_fwd_launches_ms"] - res["gates_bwd_launches_ms"], 4)

# ---- R replicas in one walk next to R one-replica walks
ones = [gate[k:k + 1].contiguous() for k in range(R)]
_, res["walk_1_replica_x%d_ms" % R], _ = timed(lambda: [walk(g) for g in ones])
res["one_replica_walks_over_stacked_walk"] = round(res["walk_1_replica_x%d_ms" % R] / res["walk_ms"], 3)

# ---- what the defaults select: per lambda its own mask, then the selection, then the best four paths' facts
mk, res["learn_mask_ms"], res["learn_mask_ms_min"] = timed(lambda: rd.learn_mask(model, iterations=ITERATIONS), 2)
ok = (short.reached & (scale > 0)).cpu().numpy()
n_free = mk.n_free.double().cpu().numpy()
per_lambda = []
for k, lam in enumerate(LAMBDAS):
    keep_k = torch.where(free, mk.replica_gate[k] > 0.5, torch.ones_like(free))
    kept_k = rd.rescore(model, keep=keep_k).score
    gap = ((kept_k - mk.target).abs() / scale.clamp(min=1e-30)).double().cpu().numpy()[ok]
    hard_gap = ((mk.replica_hard_score[k] - mk.target).abs() / scale.clamp(min=1e-30)).double().cpu().numpy()[ok]
    frac = (mk.replica_size[k].double().cpu().numpy() / np.maximum(n_free, 1))[ok]
    per_lambda.append(dict(lam=lam, size_over_n_free_mean=round(float(frac.mean()), 4), kept_gap_over_scale_mean=round(float(gap.mean()), 4),
                           kept_gap_over_scale_median=round(float(np.median(gap)), 4), hard_gap_over_scale_mean=round(float(hard_gap.mean()), 4),
                           rows_chosen=int((mk.replica == k).sum().item())))
res["per_lambda"] = per_lambda
sel_gap = (mk.sufficiency_gap().abs() / scale.clamp(min=1e-30)).double().cpu().numpy()[ok]
paths = rd.top_paths(4)
keep_p = paths.fact_mask(4) | ~free
only = rd.rescore(model, keep=keep_p)
path_gap = ((mk.target - only.score).abs() / scale.clamp(min=1e-30)).double().cpu().numpy()[ok]
path_size = torch.zeros(B, device="cuda", dtype=torch.int64).index_add_(0, row, (keep_p & free).long()).double().cpu().numpy()[ok]
res.update(rows_compared=int(ok.sum()), mask_size_mean=round(float(mk.size.double().cpu().numpy()[ok].mean()), 3),
           mask_size_over_n_free_mean=round(float((mk.size.double().cpu().numpy() / np.maximum(n_free, 1))[ok].mean()), 4),
           mask_gap_over_scale_mean=round(float(sel_gap.mean()), 4), mask_gap_over_scale_median=round(float(np.median(sel_gap)), 4),
           paths4_size_mean=round(float(path_size.mean()), 3), paths4_gap_over_scale_mean=round(float(path_gap.mean()), 4),
           paths4_gap_over_scale_median=round(float(np.median(path_gap)), 4),
           mask_closer_than_paths4=round(float((sel_gap < path_gap).mean()), 4))
line = json.dumps(res)
print(line)
with open(out_path, "w") as fh:
    fh.write(line + "\n")
