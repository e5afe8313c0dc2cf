"""Cost of extrapolation.T_RED_GNN.attention_profile on synthetic.make_extrapolation_shape("X"): one JSON line with, per hop, the
time of the profile kernel (HIP events around rg_xattn_profile) next to the forward's layer kernel (rg_xlayer_fwd) of the same call, and
the bin path the kernel took by the formula of csrc/profile.hip.  After a warm-up call, `reps` calls; median, min and max per hop.

    python tools/probe_extrap_profile.py X 64 > profiles/xattn_profile_X_B64.json
    python tools/probe_extrap_profile.py X 64 [reps] [attn_dim] [lds_budget_kib]

``attn_dim`` overrides the shape's attention width (X has 30, padded to 32; the reference's ICEWS14 default pads to 8);
``lds_budget_kib`` names the budget of a variant build (-DRG_XPF_LDS_KIB=..., loaded through RG_LIB) so that the reported path is that
build's.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from red_gnn_amd import engine                                   # noqa: E402
from red_gnn_amd import extrapolation as X                        # noqa: E402
from red_gnn_amd import profile as P                              # noqa: E402
from red_gnn_amd.models import pad_attn                           # noqa: E402
from red_gnn_amd.synthetic import SHAPES, make_extrapolation_shape   # noqa: E402


def main():
    cfg = sys.argv[1] if len(sys.argv) > 1 else "X"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    if cfg != "X":
        raise SystemExit("probe_extrap_profile: the extrapolation shape is X (got %r)" % cfg)
    sh = SHAPES[cfg]
    attn_dim = int(sys.argv[4]) if len(sys.argv) > 4 else sh["attn_dim"]
    budget_kib = int(sys.argv[5]) if len(sys.argv) > 5 else 80
    torch.cuda.set_device(0)
    data, n_ent, n_rel, gran = make_extrapolation_shape(cfg)

    class Params:
        pass

    p = Params()
    p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = (
        n_ent, n_rel, data, gran, sh["hidden_dim"], attn_dim, sh["n_layer"], "relu", "cuda")
    torch.manual_seed(0)
    model = X.T_RED_GNN(p).cuda().eval()
    L = model.n_layer
    rng = np.random.default_rng(5)
    late = np.flatnonzero(data[:, 3] // gran >= 200)              # full 120-day windows
    q = data[np.sort(rng.choice(late, B, replace=False))]
    batch = X._Batch(q[:, 0], q[:, 1], q[:, 3])

    prof_ms, layer_ms = [], []
    for _ in range(1 + reps):                                     # the first call warms up
        engine.KERNEL_EVENTS, engine.PROFILE_EVENTS = [], []
        prof = model.attention_profile(batch)
        torch.cuda.synchronize()
        fev, pev = engine.KERNEL_EVENTS, engine.PROFILE_EVENTS
        engine.KERNEL_EVENTS = engine.PROFILE_EVENTS = None
        layer_ms.append([s.elapsed_time(e) for (s, e, _, _) in fev])
        by_level = {lvl: s.elapsed_time(e) for (s, e, lvl) in pev}
        prof_ms.append([by_level[l] for l in range(1, L + 1)])
    edges_per_hop = list(model.last_stats["n_edges"])
    assert prof.count.sum((0, 2, 3)).tolist() == edges_per_hop   # the profile holds every edge the forward aggregated
    # whole calls, by device events over all repeats: the profile and the forward alone
    def mean_ms(f):
        f()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        for _ in range(reps):
            f()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps

    def forward_alone():
        with torch.no_grad():
            model._run(batch, dense=False)
    t_prof, t_fwd = mean_ms(lambda: model.attention_profile(batch)), mean_ms(forward_alone)

    layer_ms, prof_ms = np.array(layer_ms[1:]), np.array(prof_ms[1:])
    n_rows, ap, n_bins = n_rel + 2, pad_attn(attn_dim), len(P.DEFAULT_LAG_EDGES) + 1
    n_lag = model.last_stats["n_tab"]                             # one table entry per row of the forward's time table
    lds_bytes = 16384 + n_rows * (4 * ap + 12 * n_bins) + n_lag
    r3 = lambda a: [round(float(x), 4) for x in a]
    print(json.dumps(dict(
        probe="extrap_profile", cfg=cfg, B=B, n_layer=L, reps=reps, n_rela_rows=n_rows, attn_dim=attn_dim, ap=ap, hidden_dim=sh["hidden_dim"],
        n_bins=n_bins, lag_edges=list(P.DEFAULT_LAG_EDGES), lds_bytes_for_bins=lds_bytes, lds_budget_bytes=budget_kib * 1024,
        bin_path="LDS bins" if lds_bytes <= budget_kib * 1024 else "global atomics", lib=os.path.basename(os.environ.get("RG_LIB", "libredgnn.so")),
        edges_per_hop=edges_per_hop, edges_per_lag_bin=prof.count.sum((0, 1, 3)).tolist(),
        attention_profile_ms=round(t_prof, 3), forward_ms=round(t_fwd, 3),
        xattn_profile_ms_per_hop=r3(np.median(prof_ms, 0)), xattn_profile_ms_per_hop_min=r3(prof_ms.min(0)),
        xattn_profile_ms_per_hop_max=r3(prof_ms.max(0)),
        xlayer_fwd_ms_per_hop=r3(np.median(layer_ms, 0)), xlayer_fwd_ms_per_hop_min=r3(layer_ms.min(0)),
        xlayer_fwd_ms_per_hop_max=r3(layer_ms.max(0)),
        profile_over_layer_per_hop=r3(np.median(prof_ms, 0) / np.median(layer_ms, 0)))))


if __name__ == "__main__":
    main()
