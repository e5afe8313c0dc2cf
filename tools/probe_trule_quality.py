"""Cost of T_RED_GNN.rule_quality (engine.trule_ground, rg_trule_ground) on the ICEWS14-shaped synthetic of BASELINE configs[4] (C5,
synthetic.make_temporal_shape): the rules mined from held-out-style queries - base quadruples left out of the model's graph together
with their inverses - grounded on the graph's default anchors, every (head, time) of its non-identity rows.  One JSON line with the
time of the whole call, every chunk's rules, anchors, words per entity and kernel time (HIP events, engine.TRULE_EVENTS), and exact
equality with tests/trule_ground_ref.py: counts on the first 256 anchors.

For scale only, the same table (relations without their directions) grounded by engine.rule_ground on the time-stripped graph with every
entity a source: that count ignores time and has 7 000 columns where the temporal one has one per (entity, time), so the two times
compare cost, not results.

    python tools/probe_trule_quality.py [C5] [n_queries] [out.json]      # default out: profiles/trule_quality_<cfg>.json
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_temporal_shape     # noqa: E402
from red_gnn_amd.temporal import T_RED_GNN                        # noqa: E402
from tests import trule_ground_ref as T                           # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C5"
n_queries = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "trule_quality_%s.json" % cfg)
if cfg != "C5":
    raise SystemExit("probe_trule_quality: the temporal shape is C5 (got %r)" % cfg)
K, WARMUP, REPEAT, CHECK_ANCHORS = 4, 1, 3, 256
sh = SHAPES[cfg]
kg = make_temporal_shape(cfg)
rng = np.random.default_rng(0)
held_idx = np.sort(rng.choice(kg.n_base, n_queries, replace=False))
held = kg.quads[held_idx].astype(np.int64)
quads = np.delete(kg.quads, np.concatenate([held_idx, held_idx + kg.n_base]), axis=0)      # the queries and their inverses leave the graph


class P:
    pass


p = P()
p.n_rel, p.n_ent, p.n_time, p.graph = kg.n_rel - 1, kg.n_ent, kg.n_time, quads             # kg.n_rel counts the identity: the model's is one less
p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda"
torch.manual_seed(0)
model = T_RED_GNN(p).cuda().eval()
graph = model.graph


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


table = model.rules_all(held, k=K, batch_size=64)
R, L = int(table.head.numel()), int(table.body.shape[1])
anchors = graph.default_anchors()
S = len(anchors)
res = dict(cfg=cfg, n_ent=graph.n_ent, n_fact=graph.n_fact, n_time=graph.n_time, n_rela_rows=graph.n_rela_rows, n_queries=n_queries, k=K,
           n_rules=R, n_hops=L, n_anchors=S, warmup=WARMUP, repeat=REPEAT, scratch_budget=engine.RULE_SCRATCH_BYTES,
           steps_by_direction={name: int((table.direction == d).sum()) for d, name in enumerate(engine.TRULE_DIRECTIONS)})
n_r, s_c = engine.rule_chunking(graph.n_ent, R, S, engine.RULE_SCRATCH_BYTES)
res.update(rules_per_chunk=n_r, anchors_per_block=s_c, chunks=-(-R // n_r) * -(-S // s_c),
           scratch_bytes=engine.trule_ground_scratch_bytes(graph.n_ent, min(n_r, R), min(s_c, S)))
quality, res["rule_quality_ms"], res["rule_quality_ms_min"] = timed(lambda: model.rule_quality(table), WARMUP, REPEAT)
engine.TRULE_EVENTS = []
model.rule_quality(table)
torch.cuda.synchronize()
res["chunk_ms"] = [dict(n_rules=r, n_anchors=s, words_per_entity=-(-s // 32), ms=round(a.elapsed_time(b), 4))
                   for a, b, r, s in engine.TRULE_EVENTS]
res["kernel_ms_sum"] = round(sum(c["ms"] for c in res["chunk_ms"]), 4)
engine.TRULE_EVENTS = None
counts = torch.stack([quality.body_pairs, quality.hits, quality.pca_body_pairs, quality.head_pairs], 1)
res.update(body_pairs_max=int(counts[:, 0].max()), hits_sum=int(counts[:, 1].sum()), rules_with_body=int((counts[:, 0] > 0).sum()),
           rules_with_hits=int((counts[:, 1] > 0).sum()), trivial_rules=int(quality.trivial().sum()))

# ---- exact equality with the numpy reference on the first anchors (in sorted order) ------------------------------------------------
first = anchors[:CHECK_ANCHORS]
rules = tuple(x.cpu().numpy() for x in (table.head, table.body, table.direction))
got = engine.trule_ground(graph, *rules, first).cpu().numpy()
ref = T.counts(graph.n_ent, graph.n_rela_rows, graph.n_time, quads, *rules, first)
res.update(checked_anchors=len(first), exact_equal=bool(np.array_equal(got, ref)), checked_body_pairs=int(ref[:, 0].sum()))

# ---- for scale: the static grounding of the same relation sequences, time ignored ---------------------------------------------------
n_base_rel = (kg.n_rel - 1) // 2
base = quads[quads[:, 1] < n_base_rel][:, :3]
static = engine.Graph(graph.n_ent, n_base_rel, base)
assert static.n_fact == graph.n_fact
_, res["static_rule_ground_ms"], res["static_rule_ground_ms_min"] = timed(lambda: engine.rule_ground(static, table.head, table.body),
                                                                           WARMUP, REPEAT)
res["static_sources"] = static.n_ent

# ---- the lane assignment, where the hops and not the fills set the time: few entities (small bitmaps), two relation ids of a million
# edges each, and few anchors per time id, so that a "now" range is one or two words of a 256-word row.  The same eight bodies under
# every direction; run once more with RG_LIB = a build with -DRG_TRULE_ONE_G (tools/build_variant.sh) for the row-wide group throughout
from red_gnn_amd.synthetic import make_temporal_kg               # noqa: E402
hub = make_temporal_kg(2000, 1, 365, 1_000_000, seed=5)
hub_graph = engine.TemporalGraph(hub.n_ent, hub.n_rel, hub.n_time, hub.quads)
every = hub_graph.default_anchors()
few = every[::len(every) // 8192][:8192]
bodies = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
lanes = dict(n_ent=hub.n_ent, n_fact=hub_graph.n_fact, n_time=hub.n_time, n_anchors=len(few), words_per_entity=-(-len(few) // 32),
             n_rules=len(bodies), n_hops=3, default_anchors=len(every))
for d, name in enumerate(engine.TRULE_DIRECTIONS):
    c, lanes[name + "_ms"], lanes[name + "_ms_min"] = timed(
        lambda: engine.trule_ground(hub_graph, np.zeros(len(bodies), np.int64), bodies, np.full_like(bodies, d), few), WARMUP, REPEAT)
    lanes[name + "_body_pairs"] = int(c[:, 0].sum())
res["lanes"] = lanes
res["library"] = os.path.basename(os.environ.get("RG_LIB") or "libredgnn.so")
line = json.dumps(res)
print(line)
if not res["exact_equal"]:
    raise SystemExit("trule_ground and tests/trule_ground_ref.py disagree")
with open(out_path, "w") as f:
    f.write(line + "\n")
