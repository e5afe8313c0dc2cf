"""Cost of extrapolation.T_RED_GNN.rule_scores (engine.xrule_apply, rg_xrule_apply) on synthetic.make_extrapolation_shape("X"): the
lag-binned rules mined (k = 4) from queries taken from the model's own late rows are grounded on the default anchors (rule_quality) and
then applied to those queries.  One JSON line with the time of the whole call, of the seed-and-hops window and of the aggregate window
(HIP events around phases 1 and 2, engine.XRULE_APPLY_EVENTS), the work model per hop counted on the host from the same definition -
the edges walked, the day entries tested against their windows and the words of the column ranges moved - and exact equality with
tests/xrule_apply_ref.py on the first rows.

For scale only, the same rules without their lags applied by engine.rule_apply on the time-stripped graph.

Second part, the lane assignment, where the hops and not the fills set the time: 2 000 entities, two relation ids of a million rows
each over 365 days and 4 096 queries of one relation (128 words per entity) spread over every fourth day, the same eight bodies under
one lag range for every step.  Where red-gnn_amd/libredgnn_xrule_apply_one_g.so exists (bash tools/build_variant.sh xrule_apply_one_g
xrule_apply.hip -DRG_XRULE_APPLY_ONE_G: the row-wide lane group for every step) a fresh child process repeats this part with that
library, and its figures are also written to profiles/xrule_apply_<cfg>_one_g.json.

    python tools/probe_xrule_apply.py [X] [n_queries] [out.json]      # default out: profiles/xrule_apply_<cfg>.json
"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine                                        # noqa: E402
from red_gnn_amd import extrapolation as XM                           # noqa: E402
from red_gnn_amd.explain import rule_weights                          # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape, make_temporal_kg      # noqa: E402
from tests import xrule_apply_ref as XA                               # noqa: E402
from tests import xrule_ground_ref as XR                              # noqa: E402

LANES_ONLY = "--lanes-only" in sys.argv
argv = [a for a in sys.argv[1:] if a != "--lanes-only"]
cfg = argv[0] if len(argv) > 0 else "X"
n_queries = int(argv[1]) if len(argv) > 1 else 64
out_path = argv[2] if len(argv) > 2 else os.path.join(ROOT, "profiles", "xrule_apply_%s.json" % cfg)
if cfg != "X":
    raise SystemExit("probe_xrule_apply: the extrapolation shape is X (got %r)" % cfg)
K, WARMUP, REPEAT, CHECK_ROWS = 4, 1, 3, 16
VARIANT = os.path.join(ROOT, "red-gnn_amd", "libredgnn_xrule_apply_one_g.so")


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
    engine.XRULE_APPLY_EVENTS = []
    try:
        f()
        torch.cuda.synchronize()
        ev = engine.XRULE_APPLY_EVENTS
        return round(sum(a.elapsed_time(b) for a, b, _, _, _ in ev), 4), round(sum(b.elapsed_time(c) for _, b, c, _, _ in ev), 4), len(ev)
    finally:
        engine.XRULE_APPLY_EVENTS = None


def work_model(n_ent, n_rel_true, data, row_day, win_lo, win_hi, rules, rels, days):
    """Per hop, over the rules' steps: the edges the hop kernel walks, the day entries it tests against their windows and the words
    of the column ranges it moves (every run of passing entries is one range), counted per distinct (head, relation, lag range)
    from the layout engine.xrule_apply forms."""
    head, body, lag_lo, lag_hi = rules
    n_day, n_rows = len(win_lo), n_rel_true + 2
    _, q_ptr, day_ptr, day_of, day_pos = engine.xrule_query_layout(rels, days, n_rows, n_day)
    by_rel = np.argsort(data[:, 1], kind="stable")
    rel_ptr = np.searchsorted(data[by_rel, 1], np.arange(n_rel_true + 1))

    def words(lo, hi):
        return 0 if lo >= hi else ((hi - 1) >> 5) - (lo >> 5) + 1

    def step_work(h, r, lo, hi):
        k0, k1, p0 = int(day_ptr[h]), int(day_ptr[h + 1]), int(q_ptr[h])
        if k0 >= k1:
            return 0, 0, 0
        ent = day_of[k0:k1]
        col = lambda k: int(day_pos[k]) - p0
        if r == n_rel_true:                                          # the self-loops: two binary searches, one range each
            if lo > XM.WINDOW:
                return n_ent, 0, 0
            b = n_day if hi > XM.WINDOW else min(hi, n_day)
            ka, kb = k0 + int(np.searchsorted(ent, min(lo, n_day))), k0 + int(np.searchsorted(ent, b))
            return n_ent, 0, n_ent * words(col(ka), col(kb))
        tested = moved = 0
        rows = by_rel[rel_ptr[r]:rel_ptr[r + 1]]
        for j in rows.tolist():
            t0, t1 = min(row_day[j] + lo, n_day), min(row_day[j] + hi, n_day)
            ka, kb = int(np.searchsorted(ent, t0)), int(np.searchsorted(ent, t1))
            if ka >= kb:
                continue
            t = ent[ka:kb]
            ok = (win_lo[t] <= j) & (j < win_hi[t])
            tested += kb - ka
            edge = np.flatnonzero(np.diff(np.concatenate([[0], ok.astype(np.int8), [0]])))      # run starts and ends, alternating
            moved += sum(words(col(k0 + ka + a), col(k0 + ka + b)) for a, b in zip(edge[0::2].tolist(), edge[1::2].tolist()))
        return len(rows), tested, moved

    memo, work = {}, []
    for l in range(body.shape[1]):
        edges = tested = moved = 0
        for i in range(len(head)):
            key = (int(head[i]), int(body[i, l]), int(lag_lo[i, l]), int(lag_hi[i, l]))
            if key not in memo:
                memo[key] = step_work(*key)
            edges, tested, moved = edges + memo[key][0], tested + memo[key][1], moved + memo[key][2]
        work.append(dict(hop=l + 1, edges=int(edges), entries_tested=int(tested), words_moved=int(moved)))
    return work, len(memo), int(len(day_of))


def lanes_part():
    hub = make_temporal_kg(2000, 1, 365, 1_000_000, seed=5)
    rows = hub.quads[:2 * hub.n_base].astype(np.int64)                # forward rows and their inverses: relation ids 0 and 1
    rows = rows[np.argsort(rows[:, 3], kind="stable")]
    hub_day = rows[:, 3]
    g = engine.TemporalGraph(hub.n_ent, 3, len(rows) + 1, XR.graph_rows(rows, hub.n_ent, 2))
    lo_w, hi_w = XR.windows(XR.offsets(hub_day))
    rng = np.random.default_rng(6)
    B = 4096
    subs, rels = rng.integers(0, hub.n_ent, B), np.zeros(B, np.int64)
    days = rng.choice(np.arange(130, len(lo_w), 4), B)                # full windows; three days in four hold no query
    bodies = np.array([[a, b, c] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    head, weight = np.zeros(len(bodies), np.int64), np.full(len(bodies), 0.5, np.float32)
    lanes = dict(n_ent=hub.n_ent, n_fact=g.n_fact, n_day=len(lo_w), batch=B, words_per_entity=-(-B // 32), query_days=len(np.unique(days)),
                 n_rules=len(bodies), n_hops=3, library=os.path.basename(os.environ.get("RG_LIB") or "libredgnn.so"))
    for name, (lo, hi) in (("lag_0_1d", (0, 2)), ("lag_8_14d", (8, 15)), ("lag_61_120d", (61, 121)), ("any", (0, engine.XRULE_ANY_HI))):
        call = lambda: engine.xrule_apply(g, head, bodies, np.full_like(bodies, lo), np.full_like(bodies, hi), weight, subs, rels, days,
                                          hub_day, lo_w, hi_w)
        out, lanes[name + "_ms"], lanes[name + "_ms_min"] = timed(call, WARMUP, REPEAT)
        lanes[name + "_hops_ms"], lanes[name + "_aggregate_ms"], _ = windows(call)
        lanes[name + "_fired_cells"] = int((out[3] > 0).sum())
        del out
    return lanes


if LANES_ONLY:
    print(json.dumps(lanes_part()))
    raise SystemExit(0)

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
batch = XM._Batch(queries[:, 0], queries[:, 1], queries[:, 3])
q_day = queries[:, 3] // gran

table = model.rules_all(queries, k=K, batch_size=64)
quality = model.rule_quality(table)
rows, weight = rule_weights(quality)
head, body, lag_lo, lag_hi = (x.cpu().numpy()[rows] for x in (table.head, table.body) + tuple(table.lag_ranges()))
row_day = model._row_time_host
win_lo, win_hi = model.windows()
res = dict(cfg=cfg, n_ent=graph.n_ent, n_fact=graph.n_fact, n_data=model.n_data, n_day=len(win_lo), n_rela_rows=graph.n_rela_rows,
           n_queries=n_queries, k=K, n_rules_mined=int(table.head.numel()), n_rules_kept=len(rows), n_hops=int(body.shape[1]), warmup=WARMUP,
           repeat=REPEAT, scratch_budget=engine.RULE_SCRATCH_BYTES, lag_edges=list(table.lag_edges),
           steps_by_bin={("any" if b == table.any_bin else str(b)): int((table.lag_bin.cpu().numpy()[rows] == b).sum())
                         for b in range(table.any_bin + 1)})
rs, res["rule_scores_ms"], res["rule_scores_ms_min"] = timed(lambda: model.rule_scores(quality, batch), WARMUP, REPEAT)
res["hops_ms"], res["aggregate_ms"], res["calls"] = windows(lambda: model.rule_scores(quality, batch))
fired = int((rs.fired > 0).sum())
res.update(fired_cells=fired, cells=int(rs.fired.numel()),
           covered_objects=int((rs.fired[torch.arange(len(queries)), torch.as_tensor(queries[:, 2]).cuda()] > 0).sum()))
rules = (head, body, lag_lo, lag_hi)
res["work_per_hop"], res["distinct_steps"], res["query_day_entries"] = work_model(n_ent, model.n_rel_true, data, row_day, win_lo, win_hi,
                                                                                   rules, queries[:, 1], q_day)
per_rel = np.bincount(queries[:, 1], minlength=graph.n_rela_rows)
res["n_words"] = int((n_ent * ((per_rel[head] + 31) // 32)).sum())

# ---- exact equality with the numpy reference on the first rows ------------------------------------------------------------------------
first = queries[:CHECK_ROWS]
got = engine.xrule_apply(graph, *rules, weight, first[:, 0], first[:, 1], first[:, 3] // gran, row_day, win_lo, win_hi)
ref = XA.apply_lists(n_ent, model.n_rel_true, data, row_day, win_lo, win_hi, *rules, weight, first[:, 0], first[:, 1], first[:, 3] // gran)
res.update(checked_rows=len(first), exact_equal=bool(XA.same(tuple(t.cpu().numpy() for t in got), ref)),
           checked_fired_cells=int((ref[3] > 0).sum()))

# ---- for scale: the same relation sequences applied by rg_rule_apply on the time-stripped graph ---------------------------------------
n_base_rel = n_rel // 2
static = engine.Graph(n_ent, n_base_rel, data[data[:, 1] < n_base_rel][:, :3])
uniq = np.unique(np.concatenate([head[:, None], body], 1), axis=0)      # the rules without lags, (head, body) sorted; the identity is 2 * n_base_rel in both
w_static = np.full(len(uniq), 0.5, np.float32)
st, res["static_rule_apply_ms"], res["static_rule_apply_ms_min"] = timed(
    lambda: engine.rule_apply(static, uniq[:, 0], uniq[:, 1:], w_static, queries[:, 0], queries[:, 1]), WARMUP, REPEAT)
res.update(static_rules=len(uniq), static_fired_cells=int((st[3] > 0).sum()))
del st, rs, got

res["lanes"] = lanes_part()
if os.path.exists(VARIANT) and not os.environ.get("RG_LIB"):
    child = subprocess.run([sys.executable, os.path.abspath(__file__), cfg, str(n_queries), "--lanes-only"], env=dict(os.environ, RG_LIB=VARIANT),
                           capture_output=True, text=True, timeout=600)
    if child.returncode != 0:
        raise SystemExit("probe_xrule_apply: the variant run failed:\n%s" % child.stderr[-2000:])
    res["lanes_one_g"] = json.loads(child.stdout.strip().splitlines()[-1])
    with open(out_path[:-5] + "_one_g.json", "w") as f:
        f.write(json.dumps(res["lanes_one_g"]) + "\n")
res["library"] = os.path.basename(os.environ.get("RG_LIB") or "libredgnn.so")
line = json.dumps(res)
print(line)
if not res["exact_equal"]:
    raise SystemExit("xrule_apply and tests/xrule_apply_ref.py disagree")
with open(out_path, "w") as f:
    f.write(line + "\n")
