"""Filtered top-k prediction on the MI355X (-m gpu): rg_topk bit for bit against a numpy lexsort reference on seeded synthetic score
matrices (both sides of the LDS-staging boundary, ties, signed zeros, infinities, NaN, every kind of exclusion list), and
RED_GNN_trans.predict on real and synthetic KGs: no known tail, forward's scores, eval semantics, the inductive modes, consistency
with the filtered ranks of the evaluation, and the train.py --save -> predict.py command line."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _util as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 7, 64, 1000, 1024)


class P:
    def __init__(self, n_layer, hidden_dim, attn_dim, n_rel, act, dropout=0.0):
        self.n_layer, self.hidden_dim, self.attn_dim, self.n_rel, self.act, self.dropout = n_layer, hidden_dim, attn_dim, n_rel, act, dropout


# ---- numpy reference ----------------------------------------------------------------------------------------------------------------
def ref_order(row, excluded):
    """Entity ids of `row` without `excluded`, by score descending (-0 == +0, NaN last), then id ascending."""
    keep = np.ones(len(row), dtype=bool)
    keep[np.asarray(excluded, dtype=np.int64)] = False
    cand = np.nonzero(keep)[0]
    v = row[cand].astype(np.float64)
    nan = np.isnan(v)
    v = np.where(nan | (v == 0), 0.0, v)
    return cand[np.lexsort((cand, -v, nan))]


def ref_topk(scores, k, orders):
    B = scores.shape[0]
    ids = np.full((B, k), -1, np.int32)
    out = np.full((B, k), -np.inf, np.float32)
    for b in range(B):
        o = orders[b][:k]
        ids[b, :len(o)] = o
        out[b, :len(o)] = scores[b, o]
    return ids, out


def index_of(lists, keys):
    """(keys, ptr, idx) of {key: tails} (rows without a list are left out)."""
    order = np.argsort(keys)
    k_sorted = np.asarray(keys, dtype=np.int64)[order]
    tails = [np.unique(np.asarray(lists[i], dtype=np.int64)) for i in order]
    ptr = np.concatenate([[0], np.cumsum([len(t) for t in tails])]).astype(np.int64)
    idx = np.concatenate(tails).astype(np.int32) if tails else np.zeros(0, np.int32)
    return k_sorted, ptr, idx


def to_dev(index):
    return tuple(torch.as_tensor(a).cuda() for a in index)


def assert_same(got, exp, what=""):
    gi, gs = (t.cpu().numpy() for t in got)
    ei, es = exp
    assert np.array_equal(gi, ei), (what, np.argwhere(gi != ei)[:5])
    assert np.array_equal(gs.view(np.uint32), es.view(np.uint32)), (what, np.argwhere(gs.view(np.uint32) != es.view(np.uint32))[:5])


def synthetic_case(n_ent, B, seed, kmax=1024):
    """Rows of three kinds (b % 3: distinct normals, heavy ties, specials) x five kinds of exclusion (b % 5: no key, ~10 %, all but a
    few, the whole row, ~50 %)."""
    rng = np.random.default_rng(seed)
    scores = np.empty((B, n_ent), np.float32)
    lists, keys, orders = {}, [], []
    for b in range(B):
        kind = b % 3
        if kind == 0:
            row = rng.standard_normal(n_ent).astype(np.float32)
        elif kind == 1:
            row = rng.integers(0, 4, n_ent).astype(np.float32) * np.float32(0.5)
        else:
            row = rng.choice(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.5], np.float32), n_ent)
        scores[b] = row
        ex = b % 5
        if ex == 0:
            excl = np.zeros(0, np.int64)
        elif ex == 1:
            excl = rng.choice(n_ent, n_ent // 10, replace=False)
        elif ex == 2:
            excl = rng.choice(n_ent, max(0, n_ent - min(n_ent, 5)), replace=False)
        elif ex == 3:
            excl = np.arange(n_ent)
        else:
            excl = rng.choice(n_ent, n_ent // 2, replace=False)
        q = 7 * b + 3
        if ex != 0:
            lists[len(keys)] = excl
            keys.append(q)
        orders.append(ref_order(row, excl))
    q_key = np.array([7 * b + 3 for b in range(B)], np.int64)
    return scores, q_key, index_of([lists[i] for i in range(len(keys))], keys), orders


@pytest.mark.parametrize("n_ent", [1, 63, 64, 65, 1000, 16384, 32768, 32769, 40943, 300000])
def test_topk_matches_numpy_reference(n_ent):
    from red_gnn_amd import engine
    B = 15 if n_ent <= 40943 else 10
    scores, q_key, index, orders = synthetic_case(n_ent, B, seed=n_ent)
    s_d, q_d, idx_d = torch.as_tensor(scores).cuda(), torch.as_tensor(q_key).cuda(), to_dev(index)
    plain = [ref_order(scores[b], []) for b in range(B)]
    for k in KS:
        got = engine.topk(s_d, k, q_d, idx_d)
        assert_same(got, ref_topk(scores, k, orders), "n_ent=%d k=%d" % (n_ent, k))
        assert_same(engine.topk(s_d, k), ref_topk(scores, k, plain), "n_ent=%d k=%d no exclusion" % (n_ent, k))
    # the whole-row exclusion gives -1 / -inf everywhere
    got = engine.topk(s_d, 7, q_d, idx_d)
    assert (got[0][3].cpu() == -1).all() and torch.isneginf(got[1][3].cpu()).all()


@pytest.mark.parametrize("n_ent", [5000, 40943])
def test_topk_is_deterministic_and_row_independent(n_ent):
    from red_gnn_amd import engine
    B = 30
    scores, q_key, index, _ = synthetic_case(n_ent, B, seed=11)
    s_d, q_d, idx_d = torch.as_tensor(scores).cuda(), torch.as_tensor(q_key).cuda(), to_dev(index)
    for k in (10, 1000):
        a = engine.topk(s_d, k, q_d, idx_d)
        b = engine.topk(s_d, k, q_d, idx_d)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        lo = engine.topk(s_d[:13].contiguous(), k, q_d[:13].contiguous(), idx_d)
        hi = engine.topk(s_d[13:].contiguous(), k, q_d[13:].contiguous(), idx_d)
        assert torch.equal(torch.cat([lo[0], hi[0]]), a[0])
        assert torch.equal(torch.cat([lo[1], hi[1]]).view(torch.int32), a[1].view(torch.int32))


def test_topk_keys_missing_from_index_and_out_of_range_tails():
    """A row whose key is not in the index excludes nothing; known tails outside 0..n_ent-1 are ignored."""
    from red_gnn_amd import engine
    rng = np.random.default_rng(5)
    n_ent, B = 2000, 6
    scores = rng.standard_normal((B, n_ent)).astype(np.float32)
    lists = [np.array([-3, 0, 5, n_ent, n_ent + 7]), np.arange(0, n_ent, 2)]
    index = index_of(lists, [10, 20])
    q_key = np.array([10, 11, 20, 0, 1 << 40, 20], np.int64)
    got = engine.topk(torch.as_tensor(scores).cuda(), 64, torch.as_tensor(q_key).cuda(), to_dev(index))
    ex = {10: [0, 5], 20: list(range(0, n_ent, 2))}
    orders = [ref_order(scores[b], ex.get(int(q_key[b]), [])) for b in range(B)]
    assert_same(got, ref_topk(scores, 64, orders))


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _trans_model(ids, n_layer=3, d=48, a=5, act="relu", dropout=0.0):
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    loader = DataLoader(ids=ids, verbose=False)
    torch.manual_seed(1234)
    return loader, RED_GNN_trans(P(n_layer, d, a, loader.n_rel, act, dropout), loader).cuda().eval()


def _synthetic_ids(n_ent=400, n_rel=6, n_tri=4000, seed=2):
    from red_gnn_amd.synthetic import make_synthetic_kg
    kg = make_synthetic_kg(n_ent, n_rel, n_tri, seed=seed)
    return dict(n_ent=kg.n_ent, n_rel=kg.n_rel, facts=kg.facts, train=kg.train, valid=kg.valid, test=kg.test)


def _check_model_predict(model, filters, subs, rels, k, mode, n_rel):
    with torch.no_grad():
        scores = model(subs, rels, mode=mode).cpu().numpy()
    pred = model.predict(subs, rels, k=k, mode=mode)
    ids, sc = pred.ids.cpu().numpy(), pred.scores.cpu().numpy()
    assert pred.ids.dtype == torch.int64 and pred.scores.dtype == torch.float32 and ids.shape == (len(subs), k)
    orders = []
    for b, (s, r) in enumerate(zip(subs.tolist(), rels.tolist())):
        known = set(filters.get((s, r), []))
        got = [int(x) for x in ids[b] if x >= 0]
        assert not known.intersection(got), (b, s, r)
        assert np.array_equal(sc[b, :len(got)].view(np.uint32), scores[b, got].view(np.uint32))
        orders.append(ref_order(scores[b], sorted(known)))
    ei, es = ref_topk(scores, k, orders)
    assert np.array_equal(ids, ei) and np.array_equal(sc.view(np.uint32), es.view(np.uint32))
    return pred, scores


@pytest.mark.parametrize("which", ["family", "synthetic"])
def test_predict_excludes_known_and_matches_forward(which):
    ids = U.load("family_ids.npz") if which == "family" else _synthetic_ids()
    loader, model = _trans_model(ids)
    q = np.array(loader.test_q[:96])
    subs, rels = q[:, 0], q[:, 1]
    for k in (1, 10, 100):
        _check_model_predict(model, loader.filters, subs, rels, k, "test", loader.n_rel)
    # exclude_known=False: the plain top-k of forward's scores
    pred = model.predict(subs, rels, k=10, exclude_known=False)
    with torch.no_grad():
        scores = model(subs, rels, mode="test").cpu().numpy()
    ei, es = ref_topk(scores, 10, [ref_order(scores[b], []) for b in range(len(subs))])
    assert np.array_equal(pred.ids.cpu().numpy(), ei) and np.array_equal(pred.scores.cpu().numpy().view(np.uint32), es.view(np.uint32))


@pytest.mark.parametrize("d,fused_dense", [(48, True), (96, True), (48, False)])
def test_predict_uses_eval_semantics_and_leaves_the_model_alone(d, fused_dense):
    """In train mode with dropout 0.3, on every forward path: the fused inference kernels (d = 48), the torch layers that d = 96 takes
    (no fused kernel at that width) and the same with the fused kernels switched off (d = 48, fused_dense = False)."""
    loader, model = _trans_model(U.load("family_ids.npz"), d=d, dropout=0.3)
    model.fused_dense = fused_dense
    q = np.array(loader.test_q[:40])
    subs, rels = q[:, 0], q[:, 1]
    with torch.no_grad():
        ref = model(subs, rels, mode="test").cpu().numpy()          # eval mode: dropout is the identity
    model.train()
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    pred = model.predict(subs, rels, k=10)
    again = model.predict(subs, rels, k=10)
    assert torch.equal(pred.ids, again.ids) and torch.equal(pred.scores.view(torch.int32), again.scores.view(torch.int32))
    assert model.training and all(m.training for m in model.modules())
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]) and p.grad is None, n
    orders = [ref_order(ref[b], loader.filters.get((int(s), int(r)), [])) for b, (s, r) in enumerate(zip(subs, rels))]
    ei, es = ref_topk(ref, 10, orders)
    assert np.array_equal(pred.ids.cpu().numpy(), ei) and np.array_equal(pred.scores.cpu().numpy().view(np.uint32), es.view(np.uint32))


def test_predict_rejects_bad_arguments():
    loader, model = _trans_model(_synthetic_ids())
    s, r = np.array([1, 2]), np.array([0, 1])
    for k in (0, 1025, -1, 2.5, True):
        with pytest.raises(ValueError):
            model.predict(s, r, k=k)
    with pytest.raises(ValueError, match="out of range"):
        model.predict(np.array([loader.n_ent]), np.array([0]))
    with pytest.raises(ValueError, match="out of range"):
        model.predict(np.array([0]), np.array([2 * loader.n_rel + 1]))
    with pytest.raises(ValueError):
        model.predict(np.array([0, 1]), np.array([0]))
    assert model.predict(s, r, k=1024).ids.shape == (2, 1024)          # k above the entities left: -1 tails
    assert (model.predict(s, r, k=1024).ids[:, loader.n_ent:] == -1).all()


def test_predict_inductive_both_modes():
    from red_gnn_amd.inductive import DataLoader
    from red_gnn_amd.models import RED_GNN_induc
    loader = DataLoader(ids=U.load("ind_WN18RR_v1_ids.npz"), verbose=False)
    torch.manual_seed(7)
    model = RED_GNN_induc(P(3, 32, 5, loader.n_rel, "tanh"), loader).cuda().eval()
    for mode, qs, filters in (("transductive", loader.valid_q, loader.val_filters), ("inductive", loader.test_q, loader.tst_filters)):
        q = np.array(qs[:64])
        _check_model_predict(model, filters, q[:, 0], q[:, 1], 10, mode, loader.n_rel)
    q = np.array(loader.valid_q[:8])
    assert model.predict(q[:, 0], q[:, 1]).ids.shape == (8, 10)       # the inductive model's default mode


def test_predict_agrees_with_filtered_ranks():
    """For an answer a of a test query with an integer filtered rank (rg_rank; no tie at a) on a row where rg_rank's shift
    s' = fl32(fl32(s - min) + 1e-8) merges no two scores: #{returned j: score_j > score_a} = min(k, rank_a - 1) when the known answers
    except a are excluded (a dropped from a copy of the index)."""
    from red_gnn_amd import engine
    from red_gnn_amd.utils import cal_ranks_csr
    loader, model = _trans_model(U.load("family_ids.npz"))
    n = 128
    subs, rels, ap, ai, fp, fi = loader.get_batch_csr(np.arange(n), data="test")
    with torch.no_grad():
        scores = model(subs, rels, mode="test")
        ranks = cal_ranks_csr(scores, ap, ai, fp, fi).double().cpu().numpy()
    S = scores.cpu().numpy()
    api, aii = ap.cpu().numpy(), ai.cpu().numpy()
    rows, lists, pairs = [], [], []
    for q in range(n):
        row = S[q]
        sh = (row - row.min()).astype(np.float32) + np.float32(1e-8)
        if len(np.unique(sh)) != len(np.unique(row)):
            continue                                    # the shift merges scores on this row
        known = loader.filters[(int(subs[q]), int(rels[q]))]
        for i in range(api[q], api[q + 1]):
            a, rank = int(aii[i]), ranks[i]
            if rank != int(rank) or (row == row[a]).sum() != 1:
                continue
            rows.append(q)
            lists.append([t for t in known if t != a])
            pairs.append((a, int(rank)))
    assert len(pairs) >= 50, len(pairs)
    rows_t = torch.as_tensor(np.array(rows)).cuda()
    sub_scores = scores[rows_t].contiguous()
    index = to_dev(index_of(lists, list(range(len(rows)))))
    q_key = torch.arange(len(rows), dtype=torch.int64).cuda()
    for k in (1, 10, 100):
        ids, sc = (t.cpu().numpy() for t in engine.topk(sub_scores, k, q_key, index))
        for p, (a, rank) in enumerate(pairs):
            sa = S[rows[p], a]
            got = int(((ids[p] >= 0) & (sc[p] > sa)).sum())
            assert got == min(k, rank - 1), (p, a, rank, k, got)


def test_train_save_then_predict_cli(tmp_path):
    ids_path = os.path.join(ROOT, "tests", "golden", "family_ids.npz")
    ckpt = str(tmp_path / "family.pt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train.py"), "--ids", ids_path, "--preset", "family", "--epochs", "1",
                        "--save", ckpt], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    c = torch.load(ckpt, map_location="cpu")
    assert set(c["opts"]) >= {"hidden_dim", "attn_dim", "n_layer", "act"} and "W_final.weight" in c["state_dict"]
    ids = U.load("family_ids.npz")
    h, rel, t = (int(x) for x in ids["test"][0])
    queries = tmp_path / "q.tsv"
    queries.write_text("%d\t%d\t?\n?\t%d\t%d\n" % (h, rel, rel, t))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "predict.py"), "--ids", ids_path, "--checkpoint", ckpt, "-k", "3",
                        "--explain", str(queries)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln and not ln.startswith("\t")]
    assert len(lines) == 6, r.stdout
    assert all(ln.split("\t")[1] in ("1", "2", "3") for ln in lines)
    assert sum(1 for ln in r.stdout.splitlines() if ln.startswith("\tpath ") or ln.startswith("\t(no path)")) == 6
    # the CLI's answers are the model's
    from red_gnn_amd.load_data import DataLoader
    from red_gnn_amd.models import RED_GNN_trans
    loader = DataLoader(ids=ids, verbose=False)
    o = c["opts"]
    model = RED_GNN_trans(P(o["n_layer"], o["hidden_dim"], o["attn_dim"], loader.n_rel, o["act"]), loader).cuda().eval()
    model.load_state_dict(c["state_dict"])
    pred = model.predict(np.array([h, t]), np.array([rel, rel + loader.n_rel]), k=3).ids.cpu().numpy()
    assert [int(ln.split("\t")[2]) for ln in lines] == pred.reshape(-1).tolist()
