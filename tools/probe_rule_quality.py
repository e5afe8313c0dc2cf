"""Cost of engine.rule_ground on the rule table of a few hundred test rows of a BASELINE shape, every entity a source: one JSON line
with the time of the whole call and of each chunk (HIP events), the chunking, and next to it the obvious torch route on the same
device for the first rules of the table - per relation a dense fp32 A_r [n_ent, n_ent], reach = (reach @ A_r > 0) from reach = A_r1
(all entities are sources, so the first product is A_r1 itself), then count_nonzero - whose counts must equal rule_ground's exactly.

    python tools/probe_rule_quality.py [C2] [n_rules] [out.json]      # default out: profiles/rule_quality_<cfg>.json
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
n_rules = int(sys.argv[2]) if len(sys.argv) > 2 else 128
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "rule_quality_%s.json" % cfg)
ROWS, BATCH, K = 256, 64, 4                   # the table: the k = 4 best paths of 256 test rows
TORCH_RULES = 16                              # rules the torch route is timed on (two n_ent^3 products each at L = 3)
WARMUP, REPEAT, TORCH_WARMUP, TORCH_REPEAT = 2, 5, 1, 3
shape = SHAPES[cfg]
kg = make_shape(cfg)
loader = DataLoader(ids=dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test), verbose=False)


class P:
    n_layer, hidden_dim, attn_dim, n_rel, act, dropout = shape["n_layer"], shape["hidden_dim"], shape["attn_dim"], kg.n_rel, "relu", 0.0


torch.manual_seed(0)
model = RED_GNN_trans(P, loader).cuda().eval()
model.use_graphs = False                       # the eager forward is what explain runs
test = np.asarray(kg.test)[:ROWS].astype(np.int64)
table = None
for lo in range(0, len(test), BATCH):
    part = model.rules(test[lo:lo + BATCH, 0], test[lo:lo + BATCH, 1], test[lo:lo + BATCH, 2], k=K)
    table = part if table is None else table + part
head, body = table.head[:n_rules].contiguous(), table.body[:n_rules].contiguous()
graph = loader.graph_for("test")
n_ent, R, L = graph.n_ent, head.numel(), body.shape[1]


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


res = dict(cfg=cfg, n_ent=n_ent, n_fact=graph.n_fact, n_rules=R, n_hops=L, n_sources=n_ent, table_rows=int(table.head.numel()),
           explained_rows=len(test), k=K, warmup=WARMUP, repeat=REPEAT, scratch_budget=engine.RULE_SCRATCH_BYTES)
n_r, s_c = engine.rule_chunking(n_ent, R, n_ent, engine.RULE_SCRATCH_BYTES)
res.update(rules_per_chunk=n_r, sources_per_block=s_c, scratch_bytes=engine.rule_ground_scratch_bytes(n_ent, min(n_r, R), min(s_c, n_ent)),
           chunks=-(-R // n_r) * -(-n_ent // s_c))
counts, res["rule_ground_ms"], res["rule_ground_ms_min"] = timed(lambda: engine.rule_ground(graph, head, body), WARMUP, REPEAT)
engine.RULE_EVENTS = []
engine.rule_ground(graph, head, body)
torch.cuda.synchronize()
res["chunk_ms"] = [dict(n_rules=r, n_sources=s, ms=round(a.elapsed_time(b), 4)) for a, b, r, s in engine.RULE_EVENTS]
engine.RULE_EVENTS = None
# the smallest source block, to see what a narrow bitmap costs: 32 sources, all rules
src32 = np.arange(32)
_, res["rule_ground_32_sources_ms"], res["rule_ground_32_sources_ms_min"] = timed(lambda: engine.rule_ground(graph, head, body, src32),
                                                                                   WARMUP, REPEAT)

# ---- the torch route on the first rules ----------------------------------------------------------------------------------------
T = min(TORCH_RULES, R)
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


head_h, body_h = head[:T].cpu().tolist(), body[:T].cpu().tolist()
for r in set(head_h) | {r for b in body_h for r in b}:
    A(r)


def torch_route():
    out = torch.zeros((T, 4), dtype=torch.int64, device="cuda")
    for i in range(T):
        reach = A(body_h[i][0])
        for r in body_h[i][1:]:
            reach = (reach @ A(r) > 0).float()
        reach, hd = reach > 0, A(head_h[i]) > 0
        out[i, 0], out[i, 1] = reach.count_nonzero(), (reach & hd).count_nonzero()
        out[i, 2], out[i, 3] = reach[hd.any(1)].count_nonzero(), hd.count_nonzero()
    return out


ref, res["torch_ms"], res["torch_ms_min"] = timed(torch_route, TORCH_WARMUP, TORCH_REPEAT)
_, res["rule_ground_same_rules_ms"], res["rule_ground_same_rules_ms_min"] = timed(lambda: engine.rule_ground(graph, head[:T], body[:T]),
                                                                                   WARMUP, REPEAT)
res.update(torch_rules=T, torch_warmup=TORCH_WARMUP, torch_repeat=TORCH_REPEAT, torch_dense_relations=len(dense),
           exact_equal=bool(torch.equal(ref, counts[:T])))
res["body_pairs_max"], res["hits_sum"] = int(counts[:, 0].max()), int(counts[:, 1].sum())
line = json.dumps(res)
print(line)
if not res["exact_equal"]:
    raise SystemExit("the torch route and rule_ground disagree")
with open(out_path, "w") as f:
    f.write(line + "\n")
