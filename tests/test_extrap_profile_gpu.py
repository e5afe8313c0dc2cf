"""extrapolation.T_RED_GNN.attention_profile on the MI355X (-m gpu): counts and alpha sums per (query | query relation, hop, lag bin,
edge relation) against a group-by over the float64 walk's edges (tests/extrap_ref.py, tests/extrap_profile_ref.py), both bin paths of
the kernel, the edge cases of a window, the bit-for-bit properties of the integer sums and the entry point's checks.

Tolerance, as tests/test_profile_gpu.py: counts exact; |sum_dev - sum_ref| <= RTOL * sum_ref + (ATOL + Q) * count per cell; cells
without edges exactly 0."""

import functools

import numpy as np
import pytest
import torch

from tests import extrap_profile_ref as XP
from tests import extrap_ref as R
from tests import profile_ref as PR
from tests.test_extrap_explain_gpu import _setup

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
Q = 2.0 ** -33
AXES = ("group", "hop", "lag", "relation")
N_ROWS = R.N_REL + 2


def _pad_attn(a):
    return (a + 3) // 4 * 4 if a <= 16 else 32


def lds_path(n_rela_rows, attn_dim, n_bins, n_lag):
    """The kernel's choice as csrc/profile.hip states it: the 16 KB head list, per relation row the a_r row (4 * ap bytes) and n_bins
    cells of 8 + 4 bytes, and the lag table, in 80 KiB of LDS."""
    return 16384 + n_rela_rows * (4 * _pad_attn(attn_dim) + 12 * n_bins) + n_lag <= 80 * 1024


def _check(prof, count_ref, sum_ref, edges, what=""):
    count, asum = prof.count.cpu().numpy(), prof.alpha_sum.cpu().numpy()
    assert prof.axes == AXES and prof.lag_edges == tuple(edges), what
    assert count.shape == count_ref.shape and count.dtype == np.int64 and asum.dtype == np.float64, what
    assert np.array_equal(count, count_ref), what
    err = np.abs(asum - sum_ref)
    bound = RTOL * sum_ref + (ATOL + Q) * count_ref
    print("%s: cells with edges %d, edges %d, largest |sum error| %.3g, largest error / bound %.3g"
          % (what, int((count_ref > 0).sum()), int(count_ref.sum()), float(err.max()),
             float((err / np.maximum(bound, 1e-300))[count_ref > 0].max(initial=0.0))))
    assert float((err - bound).max()) <= 0.0, what
    assert (asum[count_ref == 0] == 0.0).all() and (prof.fixed.cpu().numpy()[count_ref == 0] == 0).all(), what


def _against(model, q, hops, cur_t, n_rows, edges, what=""):
    """Both groupings of the profile of queries ``q`` against the walk's hops."""
    from red_gnn_amd import profile as P
    B = len(q)
    count, asum = XP.profile_cells(hops, cur_t, B, n_rows, edges)
    pq = model.attention_profile(R.Batch(q), group="query", lag_edges=edges)
    assert pq.group == "query" and pq.count.is_cuda and tuple(pq.count.shape) == (B, len(hops), len(edges) + 1, n_rows)
    _check(pq, count, asum, edges, what + " group=query")
    pr = model.attention_profile(R.Batch(q), **({} if tuple(edges) == P.DEFAULT_LAG_EDGES else {"lag_edges": edges}))      # (the defaults)
    assert pr.group == "relation" and tuple(pr.count.shape) == (n_rows, len(hops), len(edges) + 1, n_rows)
    _check(pr, *PR.by_relation(count, asum, q[:, 1], n_rows), edges, what + " group=relation")
    for frs in model._frontiers.pool.values():                   # no frontier window is left set
        assert all(getattr(fr, "_window", None) is None for fr in frs)
    return pq, pr, count


@pytest.mark.parametrize("case", range(len(R.CASES)))
def test_profile_vs_walk(case):
    from red_gnn_amd import profile as P
    d, a, act, n_layer, B = R.CASES[case]
    model, data, q, off, (_, _, hops, cur_t), _, _ = _setup(d, a, act, n_layer, B)
    assert lds_path(N_ROWS, a, 8, 16384)
    pq, pr, count = _against(model, q, hops, cur_t, N_ROWS, P.DEFAULT_LAG_EDGES, "d=%d a=%d L=%d B=%d" % (d, a, n_layer, B))
    per_bin = pq.count.sum((0, 3)).cpu().numpy()                 # [L, n_bins]
    print("edges per (hop, bin):", per_bin.tolist())
    if case < 2:
        assert (per_bin > 0).all()                               # lags past 120 occur: older rows in front of a window after empty days
    # the self-loops: relation n_rel_true, one per visited node of the level before; nothing in the row past it
    assert int(pq.count[..., R.N_REL + 1].sum()) == 0
    assert pq.count[..., R.N_REL].sum((0, 2)).cpu().numpy().tolist() == [int((h[0][:, 4] < 0).sum()) for h in hops]
    c = pq.collapse("lag")
    assert c.axes == ("group", "hop", "relation") and c.lag_edges is None and np.array_equal(c.count.cpu().numpy(), count.sum(2))
    share = pq.lag_share(0).cpu().numpy()
    assert share.shape == (n_layer, 8) and np.allclose(share.sum(1), 1.0)
    ids, mean = pq.top(0, k=3, lag=7)
    assert tuple(ids.shape) == (n_layer, 3)


def test_one_bin_per_day_refines_the_default_bins():
    from red_gnn_amd import profile as P
    d, a, act, n_layer, B = R.CASES[0]
    model, data, q, off, (_, _, hops, cur_t), _, _ = _setup(d, a, act, n_layer, B)
    daily = tuple(range(1, 122))
    assert lds_path(N_ROWS, a, 122, 16384)
    fine, _, _ = _against(model, q, hops, cur_t, N_ROWS, daily, "one bin per day")
    assert fine.count.shape[2] == 122 and len(fine.lag_labels()) == 122 and fine.lag_labels()[-1] == (121, None)
    default = model.attention_profile(R.Batch(q), group="query")
    fold = torch.as_tensor(P.lag_bins(np.arange(122), P.DEFAULT_LAG_EDGES)).cuda()
    for name in ("fixed", "count"):
        folded = torch.zeros_like(getattr(default, name)).index_add_(2, fold, getattr(fine, name))
        assert torch.equal(folded, getattr(default, name)), name
    one = model.attention_profile(R.Batch(q), group="query", lag_edges=())
    assert one.lag_edges == () and one.count.shape[2] == 1 and one.lag_labels() == [(0, None)]
    flat = default.collapse("lag")
    assert torch.equal(one.count[:, :, 0], flat.count) and torch.equal(one.fixed[:, :, 0], flat.fixed)
    assert torch.equal(one.collapse("lag").fixed, flat.fixed)


class _Params:
    """extrap_ref.Params with the graph's sizes as arguments."""

    def __init__(self, data, n_ent, n_rel, d, a, act, n_layer):
        self.n_ent, self.n_rel, self.data, self.time_granularity = n_ent, n_rel, data, 24
        self.hidden_dim, self.attn_dim, self.n_layer, self.act, self.device = d, a, n_layer, act, "cuda"


def test_both_bin_paths_give_the_walks_table():
    """1502 relation rows with 8 bins at attn_dim 8: 1502 * (32 + 96) B = 192 KB of bins, above any budget up to 160 KiB: the
    global-atomic path; 8 rows: 1 KB, the LDS path.  Same widths, depth and batch shape."""
    from red_gnn_amd import extrapolation as X
    from red_gnn_amd import profile as P
    from tests.temporal_ref import state_of
    n_ent, n_data, d, a, n_layer, B = 150, 6000, 16, 8, 2, 5
    for n_rel in (1500, 6):
        rng = np.random.default_rng(n_rel)
        w = 1.0 / np.arange(1, n_ent + 1); w /= w.sum()
        days = np.sort(rng.choice(np.delete(np.arange(220), [0, 50, 51, 120]), n_data))
        data = np.stack([rng.choice(n_ent, n_data, p=w[::-1]), rng.integers(0, n_rel, n_data), rng.choice(n_ent, n_data, p=w),
                         days * 24 + rng.integers(0, 24, n_data)], 1)
        data = data[np.argsort(data[:, 3], kind="stable")]
        data[:4, 1] = n_rel - 1                                  # the last true relation occurs
        q = data[np.sort(rng.choice(np.arange(30, n_data), B, replace=False))]
        n_rows = n_rel + 2
        lds = lds_path(n_rows, a, 8, 16384)
        path = "LDS bins" if lds else "global atomics"
        print("n_rela_rows=%d attn_dim=%d n_bins=8: %d B of bins and table rows -> %s"
              % (n_rows, a, n_rows * (4 * _pad_attn(a) + 12 * 8), path))
        assert lds == (n_rel == 6) and lds_path(n_rows, a, 8, 1) == lds
        assert n_rel == 6 or n_rows * (4 * _pad_attn(a) + 12 * 8) > 160 * 1024
        torch.manual_seed(3)
        model = X.T_RED_GNN(_Params(data, n_ent, n_rel, d, a, "relu", n_layer)).cuda().eval()
        off = X.get_time_offset_list(data, 24)
        _, _, hops, cur_t = R.walk(state_of(model), data, off, 24, n_ent, n_rel, q[:, 0], q[:, 1], q[:, 3], n_layer, "relu")
        _against(model, q, hops, cur_t, n_rows, P.DEFAULT_LAG_EDGES, path)


def test_empty_window_subject_without_rows_and_a_batch_of_one():
    from red_gnn_amd import profile as P
    d, a, act, n_layer, B = R.CASES[2]
    model, data, q0, off, _, _, _ = _setup(d, a, act, n_layer, B)
    from tests.temporal_ref import state_of
    # query 0: ts = 0, an empty window.  query 1: day 5, a subject without a row before day 5.  query 2: one of the case's queries.
    early = data[data[:, 3] // 24 < 5]
    assert len(early) > 0
    lonely = int(np.setdiff1d(np.arange(R.N_ENT), early[:, 0])[0])
    q = np.array([[int(data[9, 0]), 1, 0, 0], [lonely, 2, 0, 5 * 24], q0[1].tolist()], dtype=np.int64)
    _, _, hops, cur_t = R.walk(state_of(model), data, off, 24, R.N_ENT, R.N_REL, q[:, 0], q[:, 1], q[:, 3], n_layer, act)
    pq, _, _ = _against(model, q, hops, cur_t, N_ROWS, P.DEFAULT_LAG_EDGES, "edge cases")
    cnt = pq.count.cpu().numpy()
    for b, bin_ in ((0, 0), (1, P.lag_bins(5, P.DEFAULT_LAG_EDGES))):      # the self-loop alone: the window's first day is day 0
        want = np.zeros((n_layer, 8, N_ROWS), np.int64)
        want[:, int(bin_), R.N_REL] = 1
        assert np.array_equal(cnt[b], want), b
    assert cnt[2].sum() > n_layer
    for b in range(3):                                           # B = 1
        one, _, _ = _against(model, q[b:b + 1], _only(hops, b), cur_t[b:b + 1], N_ROWS, P.DEFAULT_LAG_EDGES, "B=1 query %d" % b)
        assert torch.equal(one.count[0], pq.count[b])


def _only(hops, b):
    """The walk's hops of query b alone, renamed query 0."""
    out = []
    for e, al, day in hops:
        m = e[:, 0] == b
        out.append((np.column_stack([np.zeros(int(m.sum()), np.int64), e[m, 1:]]), al[m], day[m]))
    return out


@functools.lru_cache(maxsize=None)
def _bits_case():
    d, a, act, n_layer, B = 32, 5, "relu", 2, 33
    data, q = R.make_case(d, B)
    model = R.make_model(data, d, a, act, n_layer)
    return model, q, n_layer, B


def _same(p, r, what):
    """Bit-for-bit equality of two profiles; prints the figures first."""
    dc, df = (p.count - r.count).abs(), (p.fixed - r.fixed).abs()
    print("%s: cells with another count %d, with another sum %d, largest |difference of sums| %d units of 2^-32"
          % (what, int((dc > 0).sum()), int((df > 0).sum()), int(df.max())))
    return torch.equal(p.count, r.count) and torch.equal(p.fixed, r.fixed)


def test_integer_sums_two_runs_a_permutation_and_arguments():
    from red_gnn_amd import profile as P
    model, q, n_layer, B = _bits_case()
    every = np.arange(B)
    prof = lambda idx, **kw: model.attention_profile(R.Batch(q[idx]), **kw)
    whole = prof(every)
    assert whole.lag_edges == P.DEFAULT_LAG_EDGES and _same(whole, prof(every), "two runs")
    perm = np.random.default_rng(0).permutation(B)
    assert _same(whole, prof(perm), "permutation")
    pq, pp = prof(every, group="query"), prof(perm, group="query")
    assert torch.equal(pq.count[perm], pp.count) and torch.equal(pq.fixed[perm], pp.fixed)
    with pytest.raises(ValueError):
        model.attention_profile_all(q[:, :3])
    with pytest.raises(ValueError):
        model.attention_profile_all(q, batch_size=0)
    with pytest.raises(ValueError):
        prof(every, group="time")
    with pytest.raises(ValueError):
        prof(every, lag_edges=(3, 3))


def test_integer_sums_across_splits_of_a_batch():
    """The tables of the parts of a batch add up to the batch's table bit for bit.  The kernel adds exact integers; its inputs are equal
    in every batch because the inference forward forms its per-row products with rg_rows_linear, whose rows do not depend on the row
    count (with the GEMM library's products, which pick their kernel by the row count, up to 75 cells differed by up to 15360 units)."""
    model, q, n_layer, B = _bits_case()
    every = np.arange(B)
    prof = lambda idx: model.attention_profile(R.Batch(q[idx]))
    whole = prof(every)
    ok = True
    for cuts in ([1], [16], [5, 6, 20], list(range(1, B))):
        acc = None
        for part in np.split(every, cuts):
            p = prof(part)
            acc = p if acc is None else acc + p
        assert torch.equal(whole.count, acc.count), cuts
        ok = _same(whole, acc, "cuts %s" % (cuts if len(cuts) < 5 else "every single query")) and ok
    every7 = model.attention_profile_all(q, batch_size=7)
    assert every7.group == "relation" and torch.equal(whole.count, every7.count)
    ok = _same(whole, every7, "attention_profile_all(batch_size=7)") and ok
    assert ok


def test_hop_L_cells_equal_explains_alphas_summed_on_the_host():
    """explain with one row per last-level entity of a query: its hop-L edges are all hop-L edges of the query, so their alphas,
    rounded and summed in int64 on the host by (lag bin, relation), are the profile's hop-L cells."""
    from red_gnn_amd import profile as P
    model, q, n_layer, B = _bits_case()
    pq = model.attention_profile(R.Batch(q), group="query")
    ok = True
    for i in (0, 1, 7):
        with torch.no_grad():
            last = model(R.Batch(q[[i]]))[1][1][:, 1]
        rd = model.explain(R.Batch(np.repeat(q[[i]], len(last), 0)), last)
        assert rd.reached.all()
        e, al, lag = rd.edges.cpu().numpy(), rd.alpha.cpu().numpy(), rd.lag().cpu().numpy().astype(np.int64)
        m = e[:, 1] == n_layer
        fx = np.rint(al[m].astype(np.float32) * np.float32(4294967296.0)).astype(np.int64)      # llrintf(alpha * 2^32), exact in fp32
        fixed = np.zeros((8, N_ROWS), np.int64)
        count = np.zeros((8, N_ROWS), np.int64)
        bins = P.lag_bins(lag[m], P.DEFAULT_LAG_EDGES)
        np.add.at(fixed, (bins, e[m, 3]), fx)
        np.add.at(count, (bins, e[m, 3]), 1)
        assert np.array_equal(count, pq.count[i, n_layer - 1].cpu().numpy()), i
        diff = np.abs(fixed - pq.fixed[i, n_layer - 1].cpu().numpy())
        print("query %d: %d hop-L edges, cells with another sum %d, largest |difference| %d units of 2^-32"
              % (i, int(m.sum()), int((diff > 0).sum()), int(diff.max())))
        ok = ok and not diff.any()
    assert ok


def test_entry_point_checks_leave_the_outputs_untouched():
    from red_gnn_amd import _lib, engine
    d, a, act, n_layer, B = R.CASES[2]
    model, data = _setup(d, a, act, n_layer, B)[:2]
    L, s, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    n_ent, n_bins = R.N_ENT, 8
    sg = engine.Graph(n_ent, R.N_REL // 2, data[:100, :3] % np.array([n_ent, R.N_REL // 2, n_ent]))
    out_s = torch.zeros((2, n_bins, N_ROWS), dtype=torch.int64, device="cuda")
    out_c = torch.zeros_like(out_s)
    f32 = torch.zeros((N_ROWS, 4), dtype=torch.float32, device="cuda")
    z = torch.zeros(2, dtype=torch.int32, device="cuda")
    day10 = z + 10                                               # the queries' day and their self-loops' day: a self-loop has lag 0
    lag_bin = torch.zeros(16, dtype=torch.uint8, device="cuda")

    def frontier(graph, window):
        fr = engine.Frontier(n_ent, 2, 3)
        fr.reset(torch.full((2,), int(data[0, 0]), dtype=torch.int32, device="cuda"))
        fr.expand(graph)
        if window:
            fr.set_window(z, z + 5, len(model.row_time))
        return fr

    def call(fr, g, lag=lag_bin, nb=n_bins, n_old=2, n_lag=16):
        return L.rg_xattn_profile(fr.handle, g.handle, 2, n_ent, 1, n_old, p(day10), p(day10), p(model.row_time), p(lag), n_lag, nb,
                                  p(f32), p(f32), p(f32), 4, p(f32), p(f32), 3, p(out_s), p(out_c), s)
    assert call(frontier(sg, True), sg) != 0 and b"row ids" in L.rg_last_error()
    assert call(frontier(model.graph, False), model.graph) != 0 and b"window" in L.rg_last_error()
    fr = frontier(model.graph, True)
    assert call(fr, model.graph, lag=None) != 0 and b"NULL" in L.rg_last_error()
    assert call(fr, model.graph, nb=0) != 0 and b"n_bins" in L.rg_last_error()
    assert call(fr, model.graph, nb=257) != 0 and b"n_bins" in L.rg_last_error()
    assert call(fr, model.graph, n_lag=0) != 0 and b"n_lag" in L.rg_last_error()
    assert call(fr, model.graph, n_old=3) != 0 and b"n_old" in L.rg_last_error()
    torch.cuda.synchronize()
    assert (out_s == 0).all() and (out_c == 0).all()
    # a table entry outside the bins drops its edges and nothing else: here the two self-loops (lag 0); the subject's rows among the
    # window's five (days 1.., lags below 10) stay
    assert (model.row_time[:5] < 10).all()
    lag_bin[0] = 200
    assert call(fr, model.graph) == 0
    torch.cuda.synchronize()
    kept = int(out_c.sum())
    lag_bin[0] = 0
    out_s.zero_(); out_c.zero_()
    assert call(fr, model.graph) == 0
    torch.cuda.synchronize()
    assert kept >= 2 and int(out_c.sum()) == kept + 2 and int(out_c[:, 0, R.N_REL].sum()) == 2
    fr.set_window(None, None, 0)
