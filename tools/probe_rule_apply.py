"""Cost of engine.rule_apply on a BASELINE shape: the rule table of a few hundred test rows, weighted by its confidences, applied to a
batch of test queries.  One JSON line with the time of the whole call, of seed + hops and of the aggregate per call (HIP events), the
words a hop moves, and next to it the obvious torch route on the same device - per relation a dense fp32 A_r [n_ent, n_ent], per rule
reach = (reach @ A_r > 0) from the subjects' unit rows, then the same fold of the weights - whose four outputs must equal
rule_apply's exactly.

    python tools/probe_rule_apply.py [C2] [n_queries] [out.json]      # default out: profiles/rule_apply_<cfg>.json
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd import explain                                  # noqa: E402
from red_gnn_amd.load_data import DataLoader                      # noqa: E402
from red_gnn_amd.models import RED_GNN_trans                      # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_shape              # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C2"
n_queries = int(sys.argv[2]) if len(sys.argv) > 2 else 128
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rule_apply_%s.json" % cfg)
ROWS, BATCH, K = 256, 64, 4                   # the table: the k = 4 best paths of 256 valid rows
WARMUP, REPEAT, TORCH_WARMUP, TORCH_REPEAT = 2, 5, 1, 3
shape = SHAPES[cfg]
kg = make_shape(cfg)
loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test), verbose=False)


class P:
    n_layer, hidden_dim, attn_dim, n_rel, act, dropout = shape["n_layer"], shape["hidden_dim"], shape["attn_dim"], kg.n_rel, "relu", 0.0


torch.manual_seed(0)
model = RED_GNN_trans(P, loader).cuda().eval()
model.use_graphs = False                       # the eager forward is what explain runs
valid = np.asarray(kg.valid)[:ROWS].astype(np.int64)
table = None
for lo in range(0, len(valid), BATCH):
    part = model.rules(valid[lo:lo + BATCH, 0], valid[lo:lo + BATCH, 1], valid[lo:lo + BATCH, 2], k=K)
    table = part if table is None else table + part
quality = model.rule_quality(table)
rows, weight = explain.rule_weights(quality)
head, body = table.head.cpu().numpy()[rows], table.body.cpu().numpy()[rows]
test = np.asarray(kg.test)[:n_queries].astype(np.int64)
subs, rels = test[:, 0], test[:, 1]
graph = loader.graph_for("test")
n_ent, R, L, B = graph.n_ent, len(head), body.shape[1], len(subs)


def timed(f, warmup, repeat):
    """(last result, median and minimum ms over ``repeat`` runs after ``warmup``, by device events)."""
    ms = []
    for i in range(warmup + repeat):
        s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = f()
        t.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(s.elapsed_time(t))
    return out, round(float(np.median(ms)), 4), round(min(ms), 4)


per_rel = np.bincount(rels, minlength=2 * kg.n_rel + 1)
words = n_ent * ((per_rel[head] + 31) // 32)
chunks = engine.rule_apply_chunking(words, engine.RULE_SCRATCH_BYTES)
res = dict(cfg=cfg, n_ent=n_ent, n_fact=graph.n_fact, n_rules=R, n_hops=L, n_queries=B, table_rows=int(table.head.numel()),
           explained_rows=len(valid), k=K, warmup=WARMUP, repeat=REPEAT, scratch_budget=engine.RULE_SCRATCH_BYTES, calls=len(chunks),
           slab_words=int(words.sum()), rules_with_queries=int((words > 0).sum()), output_bytes=16 * B * n_ent)
apply = lambda: engine.rule_apply(graph, head, body, weight, subs, rels)
got, res["rule_apply_ms"], res["rule_apply_ms_min"] = timed(apply, WARMUP, REPEAT)
engine.RULE_APPLY_EVENTS = []
apply()
torch.cuda.synchronize()
res["call_ms"] = [dict(n_rules=r, n_words=w, seed_hops_ms=round(a.elapsed_time(b), 4), aggregate_ms=round(b.elapsed_time(c), 4))
                  for a, b, c, r, w in engine.RULE_APPLY_EVENTS]
engine.RULE_APPLY_EVENTS = None
# words a hop moves: per rule, the edges of the step's relation times the words of the rule's rows (read; non-zero ones are ORed too)
rel_ptr = np.concatenate([[0], np.cumsum(np.bincount(graph.export()[1][:, 0], minlength=2 * kg.n_rel + 1))])
edges_of = np.diff(rel_ptr)
res["hop_words"] = [int((edges_of[body[:, l]] * (words // n_ent)).sum()) for l in range(L)]

# ---- the torch route ------------------------------------------------------------------------------------------------------------
out_ptr, out_rt, _, _ = graph.export()
rows_h = np.repeat(np.arange(n_ent), np.diff(out_ptr))
dense = {}


def A(r):
    if r not in dense:
        m = out_rt[:, 0] == r
        a = torch.zeros((n_ent, n_ent), dtype=torch.float32, device="cuda")
        a[torch.as_tensor(rows_h[m]).cuda(), torch.as_tensor(out_rt[m, 1].astype(np.int64)).cuda()] = 1.0
        dense[r] = a
    return dense[r]


for r in {int(r) for b in body for r in b}:
    A(r)
q_of = [torch.as_tensor(np.nonzero(rels == h)[0]).cuda() for h in head]
s_of = [torch.as_tensor(subs[rels == h]).cuda() for h in head]
miss = (np.float32(1.0) - weight).astype(np.float32)


def torch_route():
    best = torch.zeros((B, n_ent), dtype=torch.float32, device="cuda")
    surv = torch.ones_like(best)
    rule = torch.full((B, n_ent), -1, dtype=torch.int32, device="cuda")
    fired = torch.zeros((B, n_ent), dtype=torch.int32, device="cuda")
    for i in range(R):
        if q_of[i].numel() == 0:
            continue
        reach = A(int(body[i][0]))[s_of[i]]
        for r in body[i][1:]:
            reach = (reach @ A(int(r)) > 0).float()
        fire = torch.zeros((B, n_ent), dtype=torch.bool, device="cuda")
        fire[q_of[i]] = reach > 0
        fired += fire
        surv = torch.where(fire, surv * float(miss[i]), surv)
        better = fire & (best < float(weight[i]))
        best = torch.where(better, torch.full_like(best, float(weight[i])), best)
        rule = torch.where(better, torch.full_like(rule, i), rule)
    return best, surv, rule, fired


ref, res["torch_ms"], res["torch_ms_min"] = timed(torch_route, TORCH_WARMUP, TORCH_REPEAT)
res.update(torch_warmup=TORCH_WARMUP, torch_repeat=TORCH_REPEAT, torch_dense_relations=len(dense),
           exact_equal=bool(all(torch.equal(a, b) for a, b in zip(ref, got))))
res["cells_reached"], res["cells_fired_twice"] = int((got[3] > 0).sum()), int((got[3] > 1).sum())
line = json.dumps(res)
print(line)
if not res["exact_equal"]:
    raise SystemExit("the torch route and rule_apply disagree")
with open(out_path, "w") as f:
    f.write(line + "\n")
