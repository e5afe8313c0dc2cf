"""Cost of T_RED_GNN.rule_scores (engine.trule_apply, rg_trule_apply) on the ICEWS14-shaped synthetic of BASELINE configs[4] (C5,
synthetic.make_temporal_shape): base quadruples are held out of the model's graph together with their inverses, the rules mined from
them (k = 4) are grounded (rule_quality) and then applied to the held-out queries.  One JSON line with the time of the whole call, of
the seed-and-hops window and of the aggregate window (HIP events around phases 1 and 2, engine.TRULE_APPLY_EVENTS), the byte model
of fills, hop reads and aggregate next to them, and exact equality with tests/trule_apply_ref.py on the first rows.

For scale only, the same rules without their directions applied by engine.rule_apply on the time-stripped graph.

Second part, the lane assignment, where the hops and not the fills set the time: 2 000 entities, two relation ids of a million edges
each, 366 time ids and 4 096 queries of one relation (128 words per entity), the same eight bodies under every direction.  Where
red-gnn_amd/libredgnn_trule_apply_one_g.so exists (bash tools/build_variant.sh trule_apply_one_g trule_apply.hip
-DRG_TRULE_APPLY_ONE_G: the row-wide lane group for every direction) a fresh child process repeats this part with that library.

    python tools/probe_trule_apply.py [C5] [n_queries] [out.json]      # default out: profiles/trule_apply_<cfg>.json
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_temporal_kg, make_temporal_shape     # noqa: E402
from red_gnn_amd.temporal import T_RED_GNN                        # noqa: E402
from tests import rule_apply_ref as A                             # noqa: E402
from tests import trule_apply_ref as TA                           # noqa: E402

LANES_ONLY = "--lanes-only" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--lanes-only"]
cfg = argv[0] if len(argv) > 0 else "C5"
n_queries = int(argv[1]) if len(argv) > 1 else 64
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "trule_apply_%s.json" % cfg)
if cfg != "C5":
    raise SystemExit("probe_trule_apply: the temporal shape is C5 (got %r)" % cfg)
K, WARMUP, REPEAT, CHECK_ROWS = 4, 1, 3, 16
VARIANT = os.path.join(ROOT, "red-gnn_amd", "libredgnn_trule_apply_one_g.so")


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


def windows(f):
    """(seed + hops ms, aggregate ms, calls) of one run of ``f`` with the phases issued apart."""
    engine.TRULE_APPLY_EVENTS = []
    try:
        f()
        torch.cuda.synchronize()
        ev = engine.TRULE_APPLY_EVENTS
        return round(sum(a.elapsed_time(b) for a, b, _, _, _ in ev), 4), round(sum(b.elapsed_time(c) for _, b, c, _, _ in ev), 4), len(ev)
    finally:
        engine.TRULE_APPLY_EVENTS = None


def byte_model(n_ent, n_fact_of, head, body, per_rel, fired):
    """Bytes the kernels move at most: the fills, the hop reads with every word of a row in range (the bound "any" reaches; the atomics
    only write the non-zero words), the aggregate's bitmap requests (one word per (query, entity, rule of its relation)) and its
    output traffic (16 B read and 16 B written per reached cell)."""
    W = (per_rel[head] + 31) // 32
    n_words = int((n_ent * W).sum())
    L = body.shape[1]
    return dict(n_words=n_words, fill_bytes=4 * n_words * (2 + (L - 1)), hop_read_bytes_bound=int(4 * (n_fact_of[body] * W[:, None]).sum()),
                aggregate_bitmap_bytes=int(4 * (per_rel[head] * n_ent).sum()), aggregate_output_bytes=32 * int(fired))


def lanes_part():
    hub = make_temporal_kg(2000, 1, 365, 1_000_000, seed=5)
    g = engine.TemporalGraph(hub.n_ent, hub.n_rel, hub.n_time, hub.quads)
    rng = np.random.default_rng(6)
    B = 4096
    subs, rels, times = rng.integers(0, hub.n_ent, B), np.zeros(B, np.int64), rng.integers(0, hub.n_time, B)
    bodies = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    head, weight = np.zeros(len(bodies), np.int64), np.full(len(bodies), 0.5, np.float32)
    n_fact_of = np.bincount(hub.quads[:, 1], minlength=hub.n_rel)
    lanes = dict(n_ent=hub.n_ent, n_fact=g.n_fact, n_time=hub.n_time, batch=B, words_per_entity=-(-B // 32), n_rules=len(bodies), n_hops=3,
                 library=os.path.basename(os.environ.get("RG_LIB") or "libredgnn.so"))
    for d, name in enumerate(engine.TRULE_DIRECTIONS):
        call = lambda: engine.trule_apply(g, head, bodies, np.full_like(bodies, d), weight, subs, rels, times)
        out, lanes[name + "_ms"], lanes[name + "_ms_min"] = timed(call, WARMUP, REPEAT)
        lanes[name + "_hops_ms"], lanes[name + "_aggregate_ms"], _ = windows(call)
        lanes[name + "_fired_cells"] = int((out[3] > 0).sum())
        del out
    lanes.update(byte_model(hub.n_ent, n_fact_of, head, bodies, np.bincount(rels, minlength=hub.n_rel), 0))
    return lanes


if LANES_ONLY:
    print(json.dumps(lanes_part()))
    raise SystemExit(0)

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

table = model.rules_all(held, k=K, batch_size=64)
quality = model.rule_quality(table)
batch = {"head": held[:, 0], "relation": held[:, 1], "time": held[:, 3]}
from red_gnn_amd.explain import rule_weights                      # noqa: E402
rows, weight = rule_weights(quality)
head, body, direc = (x.cpu().numpy()[rows] for x in (table.head, table.body, table.direction))
res = dict(cfg=cfg, n_ent=graph.n_ent, n_fact=graph.n_fact, n_time=graph.n_time, n_rela_rows=graph.n_rela_rows, n_queries=n_queries, k=K,
           n_rules_mined=int(table.head.numel()), n_rules_kept=len(rows), n_hops=int(body.shape[1]), warmup=WARMUP, repeat=REPEAT,
           scratch_budget=engine.RULE_SCRATCH_BYTES,
           steps_by_direction={name: int((direc == d).sum()) for d, name in enumerate(engine.TRULE_DIRECTIONS)})
rs, res["rule_scores_ms"], res["rule_scores_ms_min"] = timed(lambda: model.rule_scores(quality, batch), WARMUP, REPEAT)
res["hops_ms"], res["aggregate_ms"], res["calls"] = windows(lambda: model.rule_scores(quality, batch))
fired = int((rs.fired > 0).sum())
res.update(fired_cells=fired, cells=int(rs.fired.numel()), covered_tails=int((rs.fired[torch.arange(len(held)), torch.as_tensor(held[:, 2]).cuda()] > 0).sum()))
per_rel = np.bincount(held[:, 1], minlength=graph.n_rela_rows)
res.update(byte_model(graph.n_ent, np.bincount(quads[:, 1], minlength=graph.n_rela_rows), head, body, per_rel, fired))

# ---- exact equality with the numpy reference on the first rows ------------------------------------------------------------------------
first = held[:CHECK_ROWS]
got = engine.trule_apply(graph, head, body, direc, weight, first[:, 0], first[:, 1], first[:, 3])
ref = A.cells_to_dense(TA.apply_cells(graph.n_ent, graph.n_rela_rows, graph.n_time, quads, head, body, direc, weight, first[:, 0], first[:, 1],
                                      first[:, 3]), len(first), graph.n_ent)
res.update(checked_rows=len(first), exact_equal=bool(A.same(tuple(t.cpu().numpy() for t in got), ref)), checked_fired_cells=int((ref[3] > 0).sum()))

# ---- for scale: the same relation sequences applied by rg_rule_apply on the time-stripped graph ---------------------------------------
n_base_rel = (kg.n_rel - 1) // 2
static = engine.Graph(graph.n_ent, n_base_rel, quads[quads[:, 1] < n_base_rel][:, :3])
assert static.n_fact == graph.n_fact
uniq = np.unique(np.concatenate([head[:, None], body], 1), axis=0)                       # the rules without directions, (head, body) sorted
w_static = np.full(len(uniq), 0.5, np.float32)
st, res["static_rule_apply_ms"], res["static_rule_apply_ms_min"] = timed(
    lambda: engine.rule_apply(static, uniq[:, 0], uniq[:, 1:], w_static, held[:, 0], held[:, 1]), WARMUP, REPEAT)
res.update(static_rules=len(uniq), static_fired_cells=int((st[3] > 0).sum()))
del st, rs, got

res["lanes"] = lanes_part()
if os.path.exists(VARIANT) and not os.environ.get("RG_LIB"):
    child = subprocess.run([sys.executable, os.path.abspath(__file__), cfg, str(n_queries), "--lanes-only"], env=dict(os.environ, RG_LIB=VARIANT),
                           capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        raise SystemExit("probe_trule_apply: the variant run failed:\n%s" % child.stderr[-2000:])
    res["lanes_one_g"] = json.loads(child.stdout.strip().splitlines()[-1])
res["library"] = os.path.basename(os.environ.get("RG_LIB") or "libredgnn.so")
line = json.dumps(res)
print(line)
if not res["exact_equal"]:
    raise SystemExit("trule_apply and tests/trule_apply_ref.py disagree")
with open(out_path, "w") as f:
    f.write(line + "\n")
