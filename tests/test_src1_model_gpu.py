"""Model level, on the committed family fixture (B = 50): hop 0 takes the single-source walk (rg_layer_fwd walk 8) and the last layer
stores no state.  model(subs, rels) must give bit for bit the scores of the per-query walk forced on every hop (engine.FORCE_WALK = 1),
eagerly and replayed from the captured graph, with the same per-hop edge counts."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_family_scores_bitwise_default_plan_vs_per_query_walk_eager_and_replayed(golden_dir):
    from red_gnn_amd import engine
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    z = np.load(os.path.join(golden_dir, "family_ids.npz"))
    ids = {k: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in z.files}
    loader = DataLoader(ids=ids, verbose=False)

    class P:
        n_layer, hidden_dim, attn_dim, n_rel, act, dropout = 3, 64, 5, loader.n_rel, "relu", 0.0

    torch.manual_seed(7)
    model = RED_GNN_trans(P, loader).cuda().eval()
    subs, rels = loader.get_batch_csr(np.arange(50), data="test")[:2]
    runs, stats = {}, {}
    try:
        with torch.no_grad():
            for tag, walk, graphs in (("walk1", 1, False), ("plan", 0, False)):
                engine.FORCE_WALK = walk
                model.use_graphs = graphs
                runs[tag] = model(subs, rels, mode="test").clone()
                stats[tag] = list(model.last_stats["n_edges"])
            engine.FORCE_WALK = 0
            model.use_graphs = True
            replayed = [model(subs, rels, mode="test").clone() for _ in range(4)]     # eager, eager, capture + replay, replay
            stats["replay"] = list(model.last_stats["n_edges"])
            assert len(model._graphed) == 1, "the forward was not captured"
            hints = next(iter(model._graphed.values())).hints
            assert hints[0][1] == 8 and all(h[1] != 8 for h in hints[1:]), hints
    finally:
        engine.FORCE_WALK = 0
    assert runs["plan"].abs().sum() > 0
    assert torch.equal(runs["plan"], runs["walk1"]), "default plan differs bitwise from the per-query walk"
    for r in replayed:
        assert torch.equal(r, runs["plan"]), "replayed forward differs bitwise from the eager one"
    assert stats["plan"] == stats["walk1"] == [int(e) for e in stats["replay"]]
