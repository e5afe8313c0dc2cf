"""Cost and outcome of TIED edge masks on one explained batch of a BASELINE shape (tools/probe_mask.py's batch): one JSON line with,
per tie ("fact", "relation"), the group statistics (groups, the largest group, groups cut into more than one chunk of
engine.MASK_TIE_CHUNK members), one iteration of learn_mask(tie=) taken apart - the stacked walk, rg_mask_tie_grad, rg_mask_step on the
groups, rg_mask_tie_gates - next to the same chain rule written with index_add_ (float atomics: no fixed bits) and with
explain._segment_sums (a padded [groups, largest group] matrix per replica), and the milliseconds per iteration of the tied driver next
to the untied one; then what the defaults select with tie="fact" next to untied learn_mask: facts in the mask and the sufficiency
gap.  The case for the kernels is fixed bits and bounded memory, not speed: the numbers say how much of an iteration they are.  HIP
events, medians (and minima) of REPEAT runs after WARMUP, one process.

    python tools/probe_mask_tie.py C2 64 [out.json]        (default: profiles/mask_tie_<cfg>_B<batch>.json)
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
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "mask_tie_%s_B%d.json" % (cfg, B))
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
           lambdas=list(LAMBDAS), n_edges=int(E), reached=int(rd.reached.sum().item()), chunk=engine.MASK_TIE_CHUNK)
free = rd.edges[:, 3] != 2 * model.n_rel
res["free_edges"] = int(free.sum())

# ---- the untied iteration: the yardstick
short, res["untied_10_iterations_ms"], _ = timed(lambda: rd.learn_mask(model, iterations=10))
_, res["untied_0_iterations_ms"], _ = timed(lambda: rd.learn_mask(model, iterations=0))
res["untied_ms_per_iteration"] = round((res["untied_10_iterations_ms"] - res["untied_0_iterations_ms"]) / 10, 4)

S, _ = explain._gated_setup(rd, model, None, "test", "probe", {})
hops, live, reached = explain._static_hops(S, "probe")
gate = short.replica_gate.clone()
(score, _, grad), res["walk_ms"], res["walk_ms_min"] = timed(
    lambda: explain._gated_group(S, rd, model, hops, None, None, None, True, check_index=False, gate=gate, split_dense=True))
scale = (short.target - short.baseline_score).abs()
inv_scale = torch.where((scale > 0) & short.reached, 1.0 / scale, torch.zeros_like(scale))
lam_s, lam_e = torch.tensor(LAMBDAS, device="cuda"), torch.zeros(R, device="cuda")

for tie in ("fact", "relation"):
    T, t = explain.mask_groups(rd, tie, free), {}
    G = T.n_groups
    sizes = np.diff(T.grp_ptr_host)
    t.update(groups=int(G), largest_group=int(sizes.max()), mean_group=round(float(sizes.mean()), 3),
             groups_of_more_than_one_edge=int((sizes > 1).sum()), cut_groups=int((sizes > engine.MASK_TIE_CHUNK).sum()),
             scratch_bytes=int(engine._lib.lib().rg_mask_tie_grad_scratch_bytes(engine._lib.ptr(T.grp_ptr_host), G, R)),
             segment_sums_matrix_bytes_per_replica=int(G) * int(sizes.max()) * 4)
    _, t["mask_groups_ms"], _ = timed(lambda: explain.mask_groups(rd, tie, free))
    group_of_member = T.group_of.long()[T.member.long()]
    hip, t["tie_grad_ms"], t["tie_grad_ms_min"] = timed(lambda: engine.mask_tie_grad(T.grp_ptr, T.member, grad, G, grp_ptr_host=T.grp_ptr_host), 20)
    atomics, t["index_add_ms"], t["index_add_ms_min"] = timed(
        lambda: torch.zeros((R, G), device="cuda").index_add_(1, group_of_member, grad[:, T.member.long()]), 20)
    padded, t["segment_sums_ms"], t["segment_sums_ms_min"] = timed(
        lambda: torch.stack([explain._segment_sums(grad[k][T.member.long()], group_of_member, G) for k in range(R)]), 20)
    t["tie_grad_vs_index_add_max_abs_diff"] = float((hip - atomics).abs().max())
    t["tie_grad_vs_segment_sums_max_abs_diff"] = float((hip - padded).abs().max())
    n_groups = (T.row_ptr[1:] - T.row_ptr[:-1])
    inv_n = torch.where(n_groups > 0, 1.0 / n_groups.float(), torch.zeros(B, device="cuda"))
    every = torch.ones(G, dtype=torch.uint8, device="cuda")
    state = [torch.full((R, G), 2.0, device="cuda"), torch.zeros((R, G), device="cuda"), torch.zeros((R, G), device="cuda")]
    grp_gate = torch.full((R, G), 0.88, device="cuda")

    def group_step():
        th, m, v = (x.clone() for x in state)
        return engine.mask_step(T.row_ptr, every, score, short.target, inv_scale, inv_n, lam_s, lam_e, hip, th, m, v, 3, gate_out=grp_gate.clone())

    _, t["mask_step_on_groups_ms"], t["mask_step_on_groups_ms_min"] = timed(group_step, 20)
    edge_gate = gate.clone()
    _, t["tie_gates_ms"], t["tie_gates_ms_min"] = timed(lambda: engine.mask_tie_gates(T.group_of, grp_gate, edge_gate), 20)
    _, t["tied_10_iterations_ms"], _ = timed(lambda: explain.learn_mask(rd, model, iterations=10, tie=tie))
    _, t["tied_0_iterations_ms"], _ = timed(lambda: explain.learn_mask(rd, model, iterations=0, tie=tie))
    t["tied_ms_per_iteration"] = round((t["tied_10_iterations_ms"] - t["tied_0_iterations_ms"]) / 10, 4)
    t["new_launches_over_walk"] = round((t["tie_grad_ms"] + t["tie_gates_ms"]) / res["walk_ms"], 5)
    res[tie] = t

# ---- what the defaults select: tie="fact" next to the untied mask, both counted in FACTS
ok = (short.reached & (scale > 0)).cpu().numpy()
un, res["untied_learn_mask_ms"], _ = timed(lambda: rd.learn_mask(model, iterations=ITERATIONS), 2)
ti, res["fact_learn_mask_ms"], _ = timed(lambda: rd.learn_tied_mask(model, tie="fact", iterations=ITERATIONS), 2)
T = explain.mask_groups(rd, "fact", free)
first = T.member[T.grp_ptr[:-1].long()].long()
per_group = lambda x: x[T.member.long()]                       # an edge value per member, a group's members contiguous
seg = T.group_of.long()[T.member.long()]
any_kept = torch.zeros(T.n_groups, device="cuda").index_add_(0, seg, per_group(un.keep).float()) > 0
all_kept = torch.zeros(T.n_groups, device="cuda").index_add_(0, seg, (~per_group(un.keep)).float()) == 0
rows = lambda flag: torch.zeros(B, device="cuda").index_add_(0, T.group_row, flag.float()).double().cpu().numpy()[ok]
gap = lambda mk: (mk.sufficiency_gap().abs() / scale.clamp(min=1e-30)).double().cpu().numpy()[ok]
res.update(rows_compared=int(ok.sum()), facts_per_row_mean=round(float(rows(torch.ones_like(any_kept)).mean()), 3),
           untied_facts_in_mask_mean=round(float(rows(any_kept).mean()), 3),
           untied_facts_split_mean=round(float(rows(any_kept & ~all_kept).mean()), 3),       # one copy kept, another dropped
           untied_edges_in_mask_mean=round(float(un.size.double().cpu().numpy()[ok].mean()), 3),
           untied_gap_over_scale_mean=round(float(gap(un).mean()), 4), untied_gap_over_scale_median=round(float(np.median(gap(un))), 4),
           fact_facts_in_mask_mean=round(float(ti.size.double().cpu().numpy()[ok].mean()), 3),
           fact_gap_over_scale_mean=round(float(gap(ti).mean()), 4), fact_gap_over_scale_median=round(float(np.median(gap(ti))), 4),
           fact_copies_agree=bool(torch.equal(ti.gate[free], ti.gate[first][ti.group[free]])))
line = json.dumps(res)
print(line)
with open(out_path, "w") as fh:
    fh.write(line + "\n")
