"""Cost of extrapolation explanation fidelity on one explained batch of synthetic.make_extrapolation_shape("X"): one JSON line with the
time of extrapolation.T_RED_GNN.explain, RDigraph.top_paths(k), per hop the HIP index build (engine.digraph_hop_index,
rg_digraph_hop_index) next to explain._hop_index - the torch build the static and interpolation drivers keep - on the same inputs in the
same run, their results asserted equal before anything is timed, the rg_digraph_tlayer_fwd launch per hop, RDigraph.rescore(keep=None)
as a whole, the 2k masked rescores of T_RED_GNN.fidelity, PathSet.fact_mask and the fidelity call itself, all in one process.  Edges per
hop, the longest destination list and the chunk count per hop go with them.  HIP events, medians (and minima) of REPEAT runs after
WARMUP.  The queries are late rows of the model's own data (full 120-day windows), each with its object as the answer.

    python tools/probe_extrap_fidelity.py X 64 [out.json]      # default out: profiles/xfidelity_X_B64.json
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from red_gnn_amd import engine, explain                           # noqa: E402
from red_gnn_amd import extrapolation as XM                       # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "X"
B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "xfidelity_%s_B%d.json" % (cfg, B))
if cfg != "X":
    raise SystemExit("probe_extrap_fidelity: the extrapolation shape is X (got %r)" % cfg)
K = 4
WARMUP, REPEAT = 3, 10
sh = SHAPES[cfg]
data, n_ent, n_rel, gran = make_extrapolation_shape(cfg)


class P:
    pass


p = P()
p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = (
    n_ent, n_rel, data, gran, sh["hidden_dim"], sh["attn_dim"], sh["n_layer"], "relu", "cuda")
M = n_rel // 2                                  # the reverse of base relation r is r + M
torch.manual_seed(0)
model = XM.T_RED_GNN(p).cuda().eval()
late = np.flatnonzero(data[:, 3] // gran >= 200)                  # full 120-day windows
queries = data[np.sort(np.random.default_rng(5).choice(late, B, replace=False))]
batch, objs = XM._Batch(queries[:, 0], queries[:, 1], queries[:, 3]), queries[:, 2]


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


rd, explain_ms, explain_min = timed(lambda: model.explain(batch, objs))
L = rd.n_hops
edges_h = rd.edges.cpu().numpy()
res = dict(cfg=cfg, B=B, k=K, n_layer=L, hidden_dim=p.hidden_dim, attn_dim=p.attn_dim, inverse_offset=M, warmup=WARMUP, repeat=REPEAT,
           chunk=engine.DIGRAPH_CHUNK, n_edges=int(edges_h.shape[0]), edges_per_hop=[int((edges_h[:, 1] == l).sum()) for l in range(1, L + 1)],
           reached=int(rd.reached.sum().item()), explain_ms=explain_ms, explain_ms_min=explain_min)
paths, res["top_paths_ms"], res["top_paths_ms_min"] = timed(lambda: rd.top_paths(K))

# ---- per hop: the HIP index next to explain._hop_index on the same inputs (every edge kept), equal before they are timed
E = rd.edges.shape[0]
n_rows = model.n_rel + 1
ranges, res["hop_ranges_ms"], res["hop_ranges_ms_min"] = timed(lambda: engine.digraph_hop_ranges(rd.edges, rd.offsets, L))
e64 = rd.edges.long()
row, hop, head, rel, tail = e64.unbind(1)
kept = torch.ones(E, dtype=torch.bool, device=rd.edges.device)
keys_prev = torch.arange(B, device=rd.edges.device) * n_ent + rd.q_sub
hip_ms, hip_min, torch_ms, torch_min, torch_all_ms = [], [], [], [], []
for l in range(1, L + 1):
    live8 = torch.zeros(E, dtype=torch.uint8, device=rd.edges.device)
    live_b = torch.zeros(E, dtype=torch.bool, device=rd.edges.device)
    new = lambda: engine.digraph_hop_index(rd.edges, ranges, l, keys_prev, n_ent, n_rows, live8, None, rd.time)
    # what the older drivers do per hop around _hop_index: the E-wide nonzero, the index, the int32 copies of its arrays, the gathers
    def old():
        at = torch.nonzero((hop == l) & kept).reshape(-1)
        o = explain._hop_index("probe", l, L, at, row, head, tail, keys_prev, n_ent, live_b)
        return o, [t.to(torch.int32).contiguous() for t in (o[1], rel[o[0]], o[4])], rd.time[o[0]].contiguous(), o[3].cpu()
    got, (o, _, o_time, _) = new(), old()
    assert got[-1] == 0 and torch.equal(got[0].long(), o[0]) and torch.equal(got[1].long(), o[1]) and torch.equal(got[2].long(), rel[o[0]])
    assert torch.equal(got[3], o_time) and torch.equal(got[4], o[2]) and torch.equal(got[5], o[3]) and torch.equal(got[6].long(), o[4])
    assert torch.equal(got[7], o[5]) and torch.equal(live8.bool(), live_b)
    _, ms, mn = timed(lambda: (new(), got[5].cpu()))              # with the hop's one copy of dst_ptr, as the driver makes it
    hip_ms.append(ms); hip_min.append(mn)
    _, ms, mn = timed(old)
    torch_all_ms.append(ms)
    at_l = torch.nonzero((hop == l) & kept).reshape(-1)
    _, ms, mn = timed(lambda: explain._hop_index("probe", l, L, at_l, row, head, tail, keys_prev, n_ent, live_b))
    torch_ms.append(ms); torch_min.append(mn)
    keys_prev = got[4]
res.update(hop_index_hip_ms_per_hop=hip_ms, hop_index_hip_ms_per_hop_min=hip_min, hop_index_torch_ms_per_hop=torch_ms,
           hop_index_torch_ms_per_hop_min=torch_min, hop_index_torch_with_nonzero_and_gathers_ms_per_hop=torch_all_ms,
           hop_index_hip_over_torch=round(sum(hip_ms) / sum(torch_ms), 4),
           hop_index_hip_over_torch_with_nonzero_and_gathers=round(sum(hip_ms) / sum(torch_all_ms), 4))

# ---- rescore(keep=None): the whole call, and the message-passing launch and the index call of every hop inside it
rs, res["rescore_all_ms"], res["rescore_all_ms_min"] = timed(lambda: rd.rescore(model))
res["rescore_all_max_abs_diff_to_score"] = float((rs.score - rd.score).abs().max().item())
res["score_abs_max"] = float(rd.score.abs().max().item())
res["rescore_all_max_rel_diff_to_score"] = float(((rs.score - rd.score).abs() / rd.score.abs().clamp(min=1.0)).max().item())
res["rescore_all_over_explain"] = round(res["rescore_all_ms"] / explain_ms, 4)
per_hop, per_hop_index = [[] for _ in range(L)], [[] for _ in range(L)]
shape_per_hop = None
for i in range(WARMUP + REPEAT):
    engine.DIGRAPH_EVENTS, engine.DIGRAPH_INDEX_EVENTS = [], []
    rd.rescore(model)
    torch.cuda.synchronize()
    ev, engine.DIGRAPH_EVENTS = engine.DIGRAPH_EVENTS, None
    ev_i, engine.DIGRAPH_INDEX_EVENTS = engine.DIGRAPH_INDEX_EVENTS, None
    if i >= WARMUP:
        for l, (s, t, n_dst, n_e) in enumerate(ev):
            per_hop[l].append(s.elapsed_time(t))
        for l, (s, t, _, _) in enumerate(ev_i):
            per_hop_index[l].append(s.elapsed_time(t))
    shape_per_hop = [(n_dst, n_e) for (_, _, n_dst, n_e) in ev]
res["tlayer_ms_per_hop"] = [round(float(np.median(x)), 4) for x in per_hop]
res["tlayer_ms_per_hop_min"] = [round(min(x), 4) for x in per_hop]
res["index_ms_per_hop_inside_rescore"] = [round(float(np.median(x)), 4) for x in per_hop_index]
res["destinations_per_hop"] = [n for n, _ in shape_per_hop]
res["tlayer_share_of_rescore"] = round(sum(res["tlayer_ms_per_hop"]) / res["rescore_all_ms"], 4)
res["index_share_of_rescore"] = round(sum(res["index_ms_per_hop_inside_rescore"]) / res["rescore_all_ms"], 4)
longest, cut, chunks = [], [], []
for l in range(1, L + 1):
    e = edges_h[edges_h[:, 1] == l]
    _, counts = np.unique(e[:, 0].astype(np.int64) * n_ent + e[:, 4], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(counts)])
    n_hub, n_chunk, longest_l = engine.digraph_chunks(ptr)
    longest.append(longest_l); cut.append(n_hub); chunks.append(n_chunk)
res.update(longest_destination_per_hop=longest, cut_destinations_per_hop=cut, chunks_per_hop=chunks)

# ---- the 2k rescores of fidelity, each alone, then the masks and the call as a whole (explain + top_paths + 2k rescores + the masks)
loops = rd.edges[:, 3] == model.n_rel_true
res["self_loop_edges"] = int(loops.sum().item())
without_ms, only_ms, live_without, live_only = [], [], [], []
for j in range(1, K + 1):
    m = paths.fact_mask(j, inverse_offset=M)
    keep_wo, keep_on = ~m, m | loops
    r, ms, _ = timed(lambda: rd.rescore(model, keep=keep_wo))
    without_ms.append(ms); live_without.append(int(r.live.sum().item()))
    r, ms, _ = timed(lambda: rd.rescore(model, keep=keep_on))
    only_ms.append(ms); live_only.append(int(r.live.sum().item()))
res.update(rescore_without_ms=without_ms, rescore_only_ms=only_ms, live_edges_without=live_without, live_edges_only=live_only)
_, res["fact_mask_ms"], res["fact_mask_ms_min"] = timed(lambda: paths.fact_mask(K, inverse_offset=M))
f, res["fidelity_ms"], res["fidelity_ms_min"] = timed(lambda: model.fidelity(batch, objs, k=K, inverse_offset=M))
res["fidelity_over_explain"] = round(res["fidelity_ms"] / explain_ms, 4)
res["necessity_mean"] = [round(v, 6) for v in f.necessity().double().mean(0).tolist()]
res["sufficiency_gap_mean"] = [round(v, 6) for v in f.sufficiency_gap().double().mean(0).tolist()]
res["disconnected"] = (rd.reached[:, None] & ~f.reached_without).double().mean(0).tolist()
line = json.dumps(res)
print(line)
with open(out_path, "w") as fh:
    fh.write(line + "\n")
