"""rg_segment_rank and the extrapolation evaluation built on it (segment_rank_fil_device, T_RED_GNN.rank_batch / evaluate) on the GPU.

The yardstick is the numpy ``segment_rank_fil``, which tests/golden/extrap_rank.npz pins to the reference's own
Temporal/extrapolation/segment.py:346-387.  Every result is an integer count plus halves, so every comparison is exact."""
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

from tests import _util as U

pytestmark = pytest.mark.gpu

N_ENT = 6000
EMPTY = 10                    # the one empty segment of the edge case
ALL_EQUAL, WITH_NAN = 4, 7
# 20 segments with pairs + the empty one: around the wave (64) and the workgroup (256), long ones, and a single pair; the targets of
# segments 0, 5, 10, 15 and 20 are absent, so every length the kernel can go wrong at occurs with a target that is found
LENGTHS = [300, 1, 64, 65, 255, 33, 257, 1000, 5000, 63, 0, 17, 128, 700, 2, 513, 40, 1000, 90, 256, 256]
# known-object list length per query, (s, p) then (s, p, t): None = the query's key is absent from the index; 0 = present with an
# empty list; around the kernel's LDS staging cap of 256 entries (200, 256 below / at it; 257, 300 above: searched in memory)
SP_LEN = [300, 1, 1, 0, 200, None, 257, 300, 300, 256, 5, 1, 300, None, 2, 200, 0, 300, 257, 40, 300]
SPT_LEN = [1, 300, 300, None, 0, 257, 200, 40, 300, 1, 5, 256, None, 300, 2, 0, 300, 257, 1, 300, 12]
SHARED = (1, 2)               # these two queries share their (s, p) and their (s, p, t) key


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _index_from_lists(X, lists, n_rel_rows, n_time):
    """A KnownObjects index from {key: ascending unique objects} (a key may list nothing)."""
    keys = np.array(sorted(lists), dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum([len(lists[k]) for k in keys])]).astype(np.int64)
    idx = np.concatenate([lists[k] for k in keys] + [np.zeros(0, np.int64)]).astype(np.int32)
    return X.KnownObjects(keys, ptr, idx, n_rel_rows, n_time)


@functools.lru_cache(maxsize=None)
def _edge_case():
    """The segments, targets and known-object lists of the edge test, with the numpy segment_rank_fil results (computed once)."""
    from red_gnn_amd import extrapolation as X
    rng = np.random.default_rng(20)
    n_q = len(LENGTHS)
    assert LENGTHS[EMPTY] == 0 and n_q == len(SP_LEN) == len(SPT_LEN) == 21
    n_rel_rows, n_time = 7, 50 * 24
    sub, pre, ts = rng.integers(0, N_ENT, n_q), rng.integers(0, n_rel_rows, n_q), rng.integers(0, 50, n_q) * 24
    sub[1:3], pre[1:3], ts[1:3] = 100, 3, 240                   # SHARED
    for q in range(n_q):                                        # every other key is its query's own
        if q not in SHARED:
            sub[q] = 200 + q
    ents, scores, target, where = [], [], np.zeros(n_q, np.int64), {}
    for q, k in enumerate(LENGTHS):
        e = np.sort(rng.choice(N_ENT, k, replace=False))
        if q % 2:
            rng.shuffle(e)                                      # the kernel must not rely on the frontier's order
        v = rng.random(k).astype(np.float32)
        if q % 3 == 0:
            v = np.round(v, 1)                                  # exact ties
        if q == ALL_EQUAL:
            v[:] = 0.5
        if k == 0 or q % 5 == 0:                                # absent in every fifth segment: an entity the segment never visited
            target[q] = int(np.setdiff1d(np.arange(N_ENT), e)[rng.integers(0, N_ENT - k)])
            where[q] = None
        else:
            where[q] = (0, k - 1, k // 2)[q % 3]                # first, last, middle pair
            target[q] = e[where[q]]
        if q == WITH_NAN:
            v[(where[q] + k // 3) % k] = np.nan                 # away from the target
        ents.append(e); scores.append(v)
    assert {LENGTHS[q] for q in where if where[q] is not None} >= {1, 63, 64, 65, 255, 256, 257, 1000, 5000}
    assert sum(where[q] is None for q in where) == 5 and {0, 1, 2} <= {q % 3 for q in where if where[q] is not None}

    def lists_for(lens, key_of):
        out = {}
        for q in range(n_q):
            if lens[q] is None or key_of(q) in out:
                continue
            k, e = lens[q], ents[q]
            # entities of the segment (the better-scored ones first, so that the filter changes the rank), the target in every other
            # list, then entities the segment never visited
            take = e[np.argsort(-np.nan_to_num(scores[q]), kind="stable")][:max(k * 2 // 3, 0)] if len(e) else e
            pool = np.concatenate([[target[q]] if q % 2 == 0 else [], take, np.setdiff1d(np.arange(N_ENT), e)[:k + 1]]).astype(np.int64)
            _, first = np.unique(pool, return_index=True)
            out[key_of(q)] = np.sort(pool[np.sort(first)][:k])
            assert len(out[key_of(q)]) == k
        return out

    sp_lists = lists_for(SP_LEN, lambda q: int(sub[q] * n_rel_rows + pre[q]))
    spt_lists = lists_for(SPT_LEN, lambda q: int((sub[q] * n_rel_rows + pre[q]) * n_time + ts[q]))
    sp, spt = _index_from_lists(X, sp_lists, n_rel_rows, 0), _index_from_lists(X, spt_lists, n_rel_rows, n_time)
    lens = [len(v) for v in list(sp_lists.values()) + list(spt_lists.values())]
    assert {0, 1, 200, 256, 257, 300} <= set(lens)              # both sides of the staging cap, and the cap itself
    assert any(target[q] in sp_lists.get(int(sub[q] * n_rel_rows + pre[q]), []) for q in range(n_q) if where[q] is not None)
    # numpy reference on the segments that have pairs (its segments are the runs of column 0: it cannot express an empty one)
    full = [q for q in range(n_q) if LENGTHS[q]]
    sp2o, spt2o = defaultdict(list), defaultdict(list)
    for q in full:
        sp2o[(sub[q], pre[q])] = sp.objects(sub[q], pre[q])
        spt2o[(sub[q], pre[q], ts[q])] = spt.objects(sub[q], pre[q], ts[q])
    entities = np.concatenate([np.stack([np.full(len(ents[q]), q), ents[q]], 1) for q in full], 0)
    t = np.concatenate([scores[q] for q in full])
    with np.errstate(invalid="ignore"):
        ref = X.segment_rank_fil(t, entities, target[full], sp2o, spt2o, sub[full].tolist(), pre[full].tolist(), ts[full].tolist())
        ref_nosp = X.segment_rank_fil(t, entities, target[full], defaultdict(list), spt2o, sub[full].tolist(), pre[full].tolist(), ts[full].tolist())
    found = np.array(ref[1])
    assert found.tolist() == [where[q] is not None for q in full]
    assert np.any(ref[2][found] < ref[0][found]) and np.any(ref[3] < ref[0][found]) and np.any(ref[3] != ref[2][found])   # the filters bite
    seg_ptr = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    return dict(scores=t, ent=entities[:, 1], seg_ptr=seg_ptr, target=target, sub=sub, pre=pre, ts=ts, sp=sp, spt=spt, full=full, ref=ref,
                ref_nosp=ref_nosp)


def _expected(case, ref):
    """The numpy results spread over all 21 queries: (rank, rank_fil, rank_fil_t, found) with 1e9 / not found for the empty segment
    and rank_fil_t = 1e9 where not found (the reference's list has no entry there)."""
    n_q = len(LENGTHS)
    rank, rank_fil, rank_fil_t, found = np.full(n_q, 1e9), np.full(n_q, 1e9), np.full(n_q, 1e9), np.zeros(n_q, bool)
    full = np.array(case["full"])
    rank[full], rank_fil[full], found[full] = ref[0], ref[2], ref[1]
    rank_fil_t[full[np.array(ref[1])]] = ref[3]
    return rank, rank_fil, rank_fil_t, found


def _run_kernel(case, qs, sp="sp", spt="spt", ptr_dtype=torch.int64, rebase=True):
    """engine.segment_rank on the queries ``qs`` (contiguous) of the case: their pairs only (``rebase``) or all pairs with offsets."""
    from red_gnn_amd import engine
    lo, hi = int(case["seg_ptr"][qs[0]]), int(case["seg_ptr"][qs[-1] + 1])
    seg_ptr = case["seg_ptr"][qs[0]:qs[-1] + 2]
    if rebase:
        scores, ent, seg_ptr = case["scores"][lo:hi], case["ent"][lo:hi], seg_ptr - lo
    else:
        scores, ent = case["scores"], case["ent"]
    args = []
    for name in (sp, spt):
        ix = case[name] if name else None
        if ix is None:
            args += [None, None]
        else:
            args += [_dev(ix.query_keys(case["sub"][qs], case["pre"][qs], case["ts"][qs]), torch.int64),
                     tuple(_dev(a, d) for a, d in zip(ix, (torch.int64, torch.int64, torch.int32)))]
    out = engine.segment_rank(_dev(scores, torch.float32), _dev(ent, torch.int32), _dev(seg_ptr, ptr_dtype), _dev(case["target"][qs], torch.int32), *args)
    torch.cuda.synchronize()
    rank, rank_fil, rank_fil_t, found = (x.cpu() for x in out)
    assert rank.dtype == rank_fil.dtype == rank_fil_t.dtype == torch.float32 and found.dtype == torch.int32
    return rank.double().numpy(), rank_fil.double().numpy(), rank_fil_t.double().numpy(), found.numpy() != 0


def _assert_same(got, want, what):
    for g, w, name in zip(got, want, ("rank", "rank_fil", "rank_fil_t", "found")):
        assert np.array_equal(g, w), "%s: %s differs at queries %s: %s vs %s" % (what, name, np.flatnonzero(g != w), g[g != w], w[g != w])


def test_device_ranks_equal_the_reference_fixture():
    """extrap_rank.npz: the output of the reference's own segment_rank_fil on 40 segments of 1-29 entities with exact ties, eight
    unreached targets and filters that hide higher scores."""
    from red_gnn_amd import extrapolation as X
    fx = U.load("extrap_rank.npz")
    n_q = len(fx["target"])
    rows = lambda ptr, idx: np.array([(fx["sub"][q], fx["pre"][q], o, fx["ts"][q]) for q in range(n_q) for o in idx[ptr[q]:ptr[q + 1]]])
    sp = X.known_objects_index(rows(fx["sp_ptr"], fx["sp_idx"]), 5, False)
    spt = X.known_objects_index(rows(fx["spt_ptr"], fx["spt_idx"]), 5, True)
    for q in range(n_q):                      # the indexes hold what the reference's dictionaries held
        assert np.array_equal(sp.objects(fx["sub"][q], fx["pre"][q]), np.unique(fx["sp_idx"][fx["sp_ptr"][q]:fx["sp_ptr"][q + 1]]))
        assert np.array_equal(spt.objects(fx["sub"][q], fx["pre"][q], fx["ts"][q]), np.unique(fx["spt_idx"][fx["spt_ptr"][q]:fx["spt_ptr"][q + 1]]))
    for scores, entities in ((fx["scores"], fx["entities"]), (_dev(fx["scores"], torch.float32), _dev(fx["entities"], torch.int64))):
        rank, found, rank_fil, rank_fil_t = X.segment_rank_fil_device(scores, entities, fx["target"], sp, spt, fx["sub"], fx["pre"], fx["ts"])
        assert isinstance(found, list) and np.array_equal(np.array(found), fx["found"]) and not all(found) and any(found)
        assert rank.dtype == np.float64 and np.array_equal(rank, fx["rank"])
        assert np.array_equal(rank_fil, fx["rank_fil"])
        assert rank_fil_t.shape == fx["rank_fil_t"].shape and np.array_equal(rank_fil_t, fx["rank_fil_t"])
    with pytest.raises(ValueError):
        X.segment_rank_fil_device(fx["scores"], fx["entities"], fx["target"][:-1], sp, spt, fx["sub"], fx["pre"], fx["ts"])


def test_kernel_edges_equal_numpy_segment_rank_fil():
    """One call over 21 segments (see LENGTHS, SP_LEN, SPT_LEN and _edge_case) against the numpy function; then without the
    time-independent index (n_keys = 0), and every segment alone at B = 1 with int32 segment bounds into the whole pair arrays."""
    case = _edge_case()
    want = _expected(case, case["ref"])
    assert not want[3][EMPTY] and want[3].sum() >= 14
    qs = np.arange(len(LENGTHS))
    _assert_same(_run_kernel(case, qs), want, "one call")
    _assert_same(_run_kernel(case, qs, ptr_dtype=torch.int32), want, "one call, int32 bounds")
    nosp = _expected(case, case["ref_nosp"])
    assert np.array_equal(nosp[1], nosp[0])                      # nothing to filter: the filtered rank is the raw one
    _assert_same(_run_kernel(case, qs, sp=None), nosp, "no (s, p) index")
    from red_gnn_amd import extrapolation as X
    case_empty = dict(case, sp=X.KnownObjects(np.zeros(0), np.zeros(1), np.zeros(0), 7, 0))
    _assert_same(_run_kernel(case_empty, qs), nosp, "empty (s, p) index")
    for q in qs:
        got = _run_kernel(case, np.array([q]), ptr_dtype=torch.int32, rebase=False)
        _assert_same(got, tuple(w[q:q + 1] for w in want), "B = 1, query %d" % q)


def test_ranks_do_not_depend_on_the_batch_split():
    case = _edge_case()
    whole = _run_kernel(case, np.arange(20))
    a, b = _run_kernel(case, np.arange(7)), _run_kernel(case, np.arange(7, 20))
    for w, x, y in zip(whole, a, b):
        assert w.tobytes() == np.concatenate([x, y]).tobytes()
    _assert_same(whole, tuple(w[:20] for w in _expected(case, case["ref"])), "20 segments")


def _model_case(d, a, act, n_layer, B):
    """The small model of test_gpu_parity.test_temporal_extrapolation_vs_oracle (120 entities, 6 relations, 5000 rows with days
    without rows, hub objects and duplicate rows)."""
    from red_gnn_amd import extrapolation as X
    rng = np.random.default_rng(d + B)
    n_ent, n_rel, n = 120, 6, 5000
    days = np.sort(rng.choice(np.delete(np.arange(200), [0, 50, 51, 120]), n))
    w = 1.0 / np.arange(1, n_ent + 1); w /= w.sum()
    data = np.stack([rng.integers(0, n_ent, n), rng.integers(0, n_rel, n), rng.choice(n_ent, n, p=w), days * 24 + rng.integers(0, 24, n)], 1)
    data = data[np.argsort(data[:, 3], kind="stable")]
    data[10:14] = data[9]

    class P:
        pass

    p = P()
    p.n_ent, p.n_rel, p.data, p.time_granularity, p.hidden_dim, p.attn_dim, p.n_layer, p.act, p.device = n_ent, n_rel, data, 24, d, a, n_layer, act, "cuda"
    torch.manual_seed(3)
    model = X.T_RED_GNN(p).cuda().eval()
    q = data[np.sort(rng.choice(np.arange(30, n), B, replace=False))]
    q40 = data[np.sort(rng.choice(np.arange(30, n), 40, replace=False))]
    return X, model, data, q, q40


def _batch(q):
    class Q:
        src_idx, rel_idx, ts = q[:, 0], q[:, 1], q[:, 3]
    return Q


def _dicts(data, q):
    sp2o = {(int(s), int(r)): np.unique(data[(data[:, 0] == s) & (data[:, 1] == r), 2]) for s, r in zip(q[:, 0], q[:, 1])}
    spt2o = {(int(s), int(r), int(t)): np.unique(data[(data[:, 0] == s) & (data[:, 1] == r) & (data[:, 3] == t), 2]) for s, r, t in zip(q[:, 0], q[:, 1], q[:, 3])}
    return sp2o, spt2o


def _host_ranks(X, rb, data, q):
    sp2o, spt2o = _dicts(data, q)
    return X.segment_rank_fil(rb.soft, rb.nodes.long().cpu().numpy(), q[:, 2], sp2o, spt2o, q[:, 0].tolist(), q[:, 1].tolist(), q[:, 3].tolist())


@pytest.mark.parametrize("d,a,act,n_layer,B", [(32, 5, "tanh", 3, 9), (64, 30, "relu", 2, 40)])
def test_rank_batch_forward_and_evaluate(d, a, act, n_layer, B):
    X, model, data, q, q40 = _model_case(d, a, act, n_layer, B)
    n_ent = model.n_ent
    sp_index, spt_index = X.known_objects_index(data, 6, False), X.known_objects_index(data, 6, True)
    model.train()
    model.time_embed.eval()
    flags = [m.training for m in model.modules()]
    assert True in flags and False in flags

    # rank_batch: the four results are the host function's on the soft and nodes that the same call returned
    rb = model.rank_batch(_batch(q), q[:, 2], sp_index, spt_index)
    assert [m.training for m in model.modules()] == flags
    for t, dt in ((rb.rank, torch.float32), (rb.rank_fil, torch.float32), (rb.rank_fil_t, torch.float32), (rb.found, torch.bool),
                  (rb.soft, torch.float32), (rb.nodes, torch.int32)):
        assert t.is_cuda and t.dtype == dt and not t.requires_grad
    assert rb.rank.shape == rb.found.shape == rb.rank_fil.shape == rb.rank_fil_t.shape == (B,) and rb.nodes.shape == (rb.soft.numel(), 2)
    rank, found, rank_fil, rank_fil_t = _host_ranks(X, rb, data, q)
    found = np.array(found)
    assert found.any() and np.any(rank_fil[found] < rank[found])
    assert np.array_equal(rb.found.cpu().numpy(), found)
    assert np.array_equal(rb.rank.double().cpu().numpy(), rank) and np.array_equal(rb.rank_fil.double().cpu().numpy(), rank_fil)
    assert np.array_equal(rb.rank_fil_t.double().cpu().numpy()[found], rank_fil_t)
    assert np.all(rb.rank_fil_t.cpu().numpy()[~found] == 1e9)
    only_raw = model.rank_batch(_batch(q), q[:, 2])
    assert torch.equal(only_raw.found, rb.found) and torch.equal(only_raw.rank, only_raw.rank_fil) and torch.equal(only_raw.rank, only_raw.rank_fil_t)

    # forward: dtypes, shapes, the nodes array and the zero pattern of score_all as before the split into _run
    model.eval()
    with torch.no_grad():
        score_all, (soft, ents) = model(_batch(q))
        logits, soft2, nodes2, dense = model._run(_batch(q), dense=True)
        assert model._run(_batch(q), dense=False)[3] is None
    assert score_all.is_cuda and score_all.dtype == torch.float32 and score_all.shape == (B, n_ent) and score_all.is_contiguous()
    assert soft.is_cuda and soft.dtype == torch.float32 and soft.shape == (len(ents),)
    assert isinstance(ents, np.ndarray) and ents.dtype == np.int64 and np.array_equal(ents, rb.nodes.cpu().numpy())
    assert nodes2.dtype == torch.int32 and np.array_equal(nodes2.cpu().numpy(), ents) and logits.shape == soft2.shape == soft.shape
    visited = torch.zeros(B, n_ent, dtype=torch.bool)
    visited[ents[:, 0], ents[:, 1]] = True
    for s in (score_all.cpu(), dense.cpu()):
        assert not bool(s[~visited].any())
    assert torch.equal(dense.cpu()[ents[:, 0], ents[:, 1]], logits.cpu())
    assert np.array_equal(score_all.cpu().numpy() == 0, dense.cpu().numpy() == 0)
    model.train()
    model.time_embed.eval()

    # evaluate in batches of 7: the ranks of the batches it ran, the reference's metrics of those ranks, the flags restored
    seen = []
    inner = model.rank_batch
    model.rank_batch = lambda *args, **kw: seen.append(inner(*args, **kw)) or seen[-1]
    try:
        metrics, (e_rank, e_found, e_rank_fil, e_rank_fil_t) = model.evaluate(q40, sp_index, spt_index, batch_size=7, return_ranks=True)
    finally:
        del model.rank_batch
    assert [m.training for m in model.modules()] == flags
    assert [r.rank.numel() for r in seen] == [7, 7, 7, 7, 7, 5]
    cat = lambda f: torch.cat([f(r) for r in seen]).double().cpu().numpy()
    assert e_rank.dtype == np.float64 and e_found.dtype == np.bool_ and e_rank.shape == e_found.shape == e_rank_fil.shape == e_rank_fil_t.shape == (40,)
    assert np.array_equal(e_rank, cat(lambda r: r.rank)) and np.array_equal(e_found, cat(lambda r: r.found) != 0)
    assert np.array_equal(e_rank_fil, cat(lambda r: r.rank_fil)) and np.array_equal(e_rank_fil_t, cat(lambda r: r.rank_fil_t))
    n_same = 0
    for i, lo in enumerate(range(0, 40, 7)):                   # a second run of the same slices
        b = q40[lo:lo + 7]
        again = model.rank_batch(_batch(b), b[:, 2], sp_index, spt_index)
        assert torch.equal(again.nodes, seen[i].nodes) and torch.equal(again.found, seen[i].found)
        # (the softmax's index_add may differ in the last bit between two runs: compare the ranks of the queries where it did not)
        differs = torch.zeros(len(b), device="cuda").index_add(0, again.nodes[:, 0].long(), (again.soft != seen[i].soft).float()) > 0
        assert torch.equal(again.rank[~differs], seen[i].rank[~differs])
        n_same += int((~differs).sum())
        host = _host_ranks(X, seen[i], data, b)
        assert np.array_equal(e_rank[lo:lo + 7], host[0]) and np.array_equal(e_rank_fil[lo:lo + 7], host[2])
        assert np.array_equal(e_rank_fil_t[lo:lo + 7][np.array(host[1])], host[3])
    print("evaluate: %d of 40 queries had bitwise equal softmax scores in the second run" % n_same)
    assert e_found.any()
    # main.py:413-430 on the returned ranks (the time-filtered list holds found queries only), divided as :434-463
    r, rf, rt, n, fc = e_rank, e_rank_fil, e_rank_fil_t[e_found], 40, e_found.sum()
    want = dict(hits1=np.sum(r == 1) / n, hits3=np.sum(r <= 3) / n, hits10=np.sum(r <= 10) / n, hits_inf=fc / n, mr=np.sum(r) / n, mrr=np.sum(1 / r) / n,
                hits1_fil=np.sum(rf <= 1) / n, hits3_fil=np.sum(rf <= 3) / n, hits10_fil=np.sum(rf <= 10) / n, mrr_fil=np.sum(1 / rf) / n,
                hits1_fil_t=np.sum(rt <= 1) / n, hits3_fil_t=np.sum(rt <= 3) / n, hits10_fil_t=np.sum(rt <= 10) / n, mrr_fil_t=np.sum(1 / rt) / n,
                hits1_found=np.sum(r == 1) / fc, hits3_found=np.sum(r <= 3) / fc, hits10_found=np.sum(r <= 10) / fc,
                mr_found=np.sum(r[e_found]) / fc, mrr_found=np.sum(1 / r[e_found]) / fc)
    assert metrics["n"] == 40 and metrics["n_found"] == fc
    for k, v in want.items():
        assert abs(metrics[k] - v) <= 1e-12, k
    assert model.evaluate(q40, sp_index, spt_index, batch_size=7).keys() == metrics.keys()
    assert len(model._known_dev) == 2                           # the two indexes went to the device once
