"""Cost of extrapolation.T_RED_GNN.rule_quality (engine.xrule_ground, rg_xrule_ground) on synthetic.make_extrapolation_shape("X"): the
lag-binned rules mined (k = 4) from queries taken from the model's own late rows, grounded on the default anchors, every (subject, day)
of the data.  One JSON line with the time of the whole call, every chunk's rules, anchors, words per entity and kernel time (HIP
events, engine.XRULE_EVENTS), the work model per hop - the days the hop kernel tests against their windows and the words of the column
ranges it moves, counted on the host from the same definition - and exact equality with tests/xrule_ground_ref.py: counts on the first
256 anchors (the first days: empty windows) and on the last 256 (full windows).

For scale only, the same table (relations without their lags) grounded by engine.rule_ground on the time-stripped graph with every
entity a source: that count ignores time and windows and has 7 000 columns where this one has one per (subject, day), so the two
times compare cost, not results.

    python tools/probe_xrule_quality.py [X] [n_queries] [out.json]      # default out: profiles/xrule_quality_<cfg>.json
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                        # noqa: E402
from red_gnn_amd import extrapolation as XM                           # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape    # noqa: E402
from tests import xrule_ground_ref as XR                              # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "X"
n_queries = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "xrule_quality_%s.json" % cfg)
if cfg != "X":
    raise SystemExit("probe_xrule_quality: the extrapolation shape is X (got %r)" % cfg)
K, WARMUP, REPEAT, CHECK_ANCHORS = 4, 1, 3, 256
sh = SHAPES[cfg]
data, n_ent, n_rel, gran = make_extrapolation_shape(cfg)


class P:
    pass


p = P()
p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = (
    n_ent, n_rel, data, gran, sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda")
torch.manual_seed(0)
model = XM.T_RED_GNN(p).cuda().eval()
graph = model.graph
rng = np.random.default_rng(5)
late = np.flatnonzero(data[:, 3] // gran >= 200)                      # full 120-day windows
queries = data[np.sort(rng.choice(late, n_queries, replace=False))]


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


table = model.rules_all(queries, k=K, batch_size=64)
R, L = int(table.head.numel()), int(table.body.shape[1])
anchors = model.default_anchors()
S = len(anchors)
row_day = model._row_time_host
win_lo, win_hi = model.windows()
n_day = len(win_lo)
res = dict(cfg=cfg, n_ent=graph.n_ent, n_fact=graph.n_fact, n_data=model.n_data, n_day=n_day, n_rela_rows=graph.n_rela_rows,
           n_queries=n_queries, k=K, n_rules=R, n_hops=L, n_anchors=S, warmup=WARMUP, repeat=REPEAT, scratch_budget=engine.RULE_SCRATCH_BYTES,
           lag_edges=list(table.lag_edges),
           steps_by_bin={("any" if b == table.any_bin else str(b)): int((table.lag_bin == b).sum()) for b in range(table.any_bin + 1)})
n_r, s_c = engine.rule_chunking(graph.n_ent, R, S, engine.RULE_SCRATCH_BYTES)
res.update(rules_per_chunk=n_r, anchors_per_block=s_c, chunks=-(-R // n_r) * -(-S // s_c),
           scratch_bytes=engine.rule_ground_scratch_bytes(graph.n_ent, min(n_r, R), min(s_c, S)))
quality, res["rule_quality_ms"], res["rule_quality_ms_min"] = timed(lambda: model.rule_quality(table), WARMUP, REPEAT)
engine.XRULE_EVENTS = []
model.rule_quality(table)
torch.cuda.synchronize()
res["chunk_ms"] = [dict(n_rules=r, n_anchors=s, words_per_entity=-(-s // 32), ms=round(a.elapsed_time(b), 4))
                   for a, b, r, s in engine.XRULE_EVENTS]
res["kernel_ms_sum"] = round(sum(c["ms"] for c in res["chunk_ms"]), 4)
engine.XRULE_EVENTS = None
counts = torch.stack([quality.body_pairs, quality.hits, quality.pca_body_pairs, quality.head_pairs], 1)
res.update(body_pairs_max=int(counts[:, 0].max()), hits_sum=int(counts[:, 1].sum()), rules_with_body=int((counts[:, 0] > 0).sum()),
           rules_with_hits=int((counts[:, 1] > 0).sum()))

# ---- the work model: per hop, over the rules' steps, the days an edge tests against their windows and the words of the column ranges
# it moves (every run of passing days is one range), with all anchors in one block.  Counted per distinct (relation, lag range).
head, body = table.head.cpu().numpy(), table.body.cpu().numpy()
lag_lo, lag_hi = (x.cpu().numpy() for x in table.lag_ranges())
ptr = np.searchsorted(anchors[:, 1], np.arange(n_day + 1))
by_rel = np.argsort(data[:, 1], kind="stable")
rel_ptr = np.searchsorted(data[by_rel, 1], np.arange(n_rel + 1))
day_idx = np.arange(n_day)


def words(a, b):                                                     # words of the columns of the days [a, b)
    return 0 if ptr[a] >= ptr[b] else ((ptr[b] - 1) >> 5) - (ptr[a] >> 5) + 1


def step_work(r, lo, hi):
    if r == model.n_rel_true:                                        # the self-loops: one range of days each, no window test
        if lo > XM.WINDOW:
            return 0, 0, n_ent
        b = n_day if hi > XM.WINDOW else min(hi, n_day)
        return 0, n_ent * words(min(lo, n_day), b), n_ent
    tested = moved = 0
    rows = by_rel[rel_ptr[r]:rel_ptr[r + 1]]
    for j in rows.tolist():
        t0, t1 = min(row_day[j] + lo, n_day), min(row_day[j] + hi, n_day)
        if t0 >= t1:
            continue
        t = day_idx[t0:t1]
        ok = (win_lo[t] <= j) & (j < win_hi[t])
        tested += t1 - t0
        edge = np.flatnonzero(np.diff(np.concatenate([[0], ok.astype(np.int8), [0]])))      # run starts and ends, alternating
        moved += sum(words(t0 + a, t0 + b) for a, b in zip(edge[0::2].tolist(), edge[1::2].tolist()))
    return tested, moved, len(rows)


memo = {}
work = []
for l in range(L):
    tested = moved = edges = 0
    for i in range(R):
        key = (int(body[i, l]), int(lag_lo[i, l]), int(lag_hi[i, l]))
        if key not in memo:
            memo[key] = step_work(*key)
        tested, moved, edges = tested + memo[key][0], moved + memo[key][1], edges + memo[key][2]
    work.append(dict(hop=l + 1, edges=int(edges), days_tested=int(tested), words_moved=int(moved)))
res["work_per_hop"] = work
res["distinct_steps"] = len(memo)
res["fill_bytes_per_rule"] = int(3 * graph.n_ent * -(-min(s_c, S) // 32) * 4)

# ---- exact equality with the numpy reference on the first and the last anchors (in sorted order) ---------------------------------------
rules = (head, body, lag_lo, lag_hi)
for name, part in (("first", anchors[:CHECK_ANCHORS]), ("last", anchors[-CHECK_ANCHORS:])):
    got = engine.xrule_ground(graph, *rules, row_day, win_lo, win_hi, part).cpu().numpy()
    ref = XR.counts(n_ent, model.n_rel_true, data, row_day, win_lo, win_hi, *rules, part)
    res["exact_equal_" + name] = bool(np.array_equal(got, ref))
    res["checked_body_pairs_" + name] = int(ref[:, 0].sum())
res["checked_anchors"] = CHECK_ANCHORS
res["exact_equal"] = res["exact_equal_first"] and res["exact_equal_last"]

# ---- for scale: the static grounding of the same relation sequences, time and windows ignored -------------------------------------------
n_base_rel = n_rel // 2
static = engine.Graph(n_ent, n_base_rel, data[data[:, 1] < n_base_rel][:, :3])
_, res["static_rule_ground_ms"], res["static_rule_ground_ms_min"] = timed(lambda: engine.rule_ground(static, table.head, table.body),
                                                                           WARMUP, REPEAT)
res["static_sources"] = static.n_ent

# ---- the lane assignment, where the hops and not the fills set the time: few entities (small bitmaps), two relation ids of a million
# rows each over 365 days, and few anchors per day (8 192 in all: a day's columns are one or two words of a 256-word row).  The same
# eight bodies under one lag range for every step; run once more with RG_LIB = a build with -DRG_XRULE_ONE_G (the row-wide group for
# every step) or -DRG_XRULE_NARROW_G (one lane per edge for every data-row step), tools/build_variant.sh
from red_gnn_amd.synthetic import make_temporal_kg                    # noqa: E402
hub = make_temporal_kg(2000, 1, 365, 1_000_000, seed=5)
rows = hub.quads[:2 * hub.n_base].astype(np.int64)                    # forward rows and their inverses: relation ids 0 and 1
rows = rows[np.argsort(rows[:, 3], kind="stable")]
hub_day = rows[:, 3]
hub_graph = engine.TemporalGraph(hub.n_ent, 3, len(rows) + 1, XR.graph_rows(rows, hub.n_ent, 2))
hub_lo, hub_hi = XR.windows(XR.offsets(hub_day))
every = XR.default_anchors(rows, hub_day, hub.n_ent)
few = every[::len(every) // 8192][:8192]
bodies = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
lanes = dict(n_ent=hub.n_ent, n_fact=hub_graph.n_fact, n_day=len(hub_lo), n_anchors=len(few), words_per_entity=-(-len(few) // 32),
             n_rules=len(bodies), n_hops=3, default_anchors=len(every))
for name, (lo, hi) in (("lag_0_1d", (0, 2)), ("lag_8_14d", (8, 15)), ("lag_61_120d", (61, 121)), ("any", (0, engine.XRULE_ANY_HI))):
    c, lanes[name + "_ms"], lanes[name + "_ms_min"] = timed(
        lambda: engine.xrule_ground(hub_graph, np.zeros(len(bodies), np.int64), bodies, np.full_like(bodies, lo), np.full_like(bodies, hi),
                                    hub_day, hub_lo, hub_hi, few), WARMUP, REPEAT)
    lanes[name + "_body_pairs"] = int(c[:, 0].sum())
res["lanes"] = lanes
res["library"] = os.path.basename(os.environ.get("RG_LIB") or "libredgnn.so")
line = json.dumps(res)
print(line)
if not res["exact_equal"]:
    raise SystemExit("xrule_ground and tests/xrule_ground_ref.py disagree")
with open(out_path, "w") as f:
    f.write(line + "\n")
