"""The r-digraph hop kernels called on their own - engine.explain_seed, explain_hop, texplain_hop, xexplain_hop, explain_gather, i.e.
csrc/explain.hip's rg_explain_* / rg_texplain_* / rg_xexplain_* - against the dense reference of tests/hop_ref.py, over the case table
defined there (layer_ref's dispatch cases plus the B = 1024 and 463-relation-row cases of the profile kernel).  Per case the frontier is
expanded hop by hop (its node list must equal the CPU oracle's), and per hop:

  1. all of level l marked, tau = 0: edges, time ids / data rows, head marks and the word pointer equal the reference exactly, in order;
     as a multiset the edges are the oracle's hop
  2. |alpha - alpha64| <= C_BOUND * (1 + n0) * u * kappa + 1e-30 per edge (hop_ref.alpha_bound: layer_ref's agg bound for one term)
  3. alpha equals, as uint32, what the layer forward writes with one-hot tables, on every singleton edge (hop_ref's docstring)
  4. mark patterns (none, one node per row, half, bits 0 and 31 of the words, the first / the last word, entities outside the level) at
     tau = 0 and tau = an alpha that occurs (the median), against the reference evaluated with the device's own alphas of step 1: alpha
     is a function of (row, head, relation), so no rounding can flip a comparison
  5. the >= edge: tau = a* keeps a*'s edges, nextafter(a*) drops exactly them; +inf: nothing and no emit call; -inf: as 0
  6. rg_explain_seed against numpy: inside the level, outside it, -1 and n_ent
  7. rg_explain_gather of the hops' lists against a numpy scatter; n = 0 leaves the outputs alone
  8. two runs are bitwise equal; a row taken alone (B = 1, the same tables) gives its slice of the batch (hop_ref.SMALL)
"""

import ctypes as C
import time
import types

import numpy as np
import pytest
import torch

from tests import hop_ref as hr
from tests import layer_ref as lr
from tests.test_layer_kernels_gpu import _dev, _extra, _forward, _setup

pytestmark = pytest.mark.gpu

# worst |alpha - alpha64| / ((1 + n0) u kappa) per entry point over the table, as measured on an MI355X (information only; the assertion
# uses C_BOUND = 1.6).  The plain fp32 numpy evaluation costs up to 0.205 as well (tests/test_hop_ref.py, ap_1 hop 2)
KERNEL_RATIOS = {"rg_explain_emit": 0.205, "rg_texplain_emit": 0.13, "rg_xexplain_emit": 0.139}
# wall time of this file on an MI355X: 6.4 s (28 tests, 3.4 s of it inside the tests; the slowest, tickets, 0.7 s)

ENTRY = {"static": "rg_explain", "temporal": "rg_texplain", "windowed": "rg_xexplain"}
ATTN = ("a_s", "a_r", "a_q", "w_alpha", "b_alpha")


def _marks_dev(m):
    return torch.as_tensor(np.ascontiguousarray(m, np.uint32).view(np.int32)).cuda()


def _marks_np(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint32)


def explain(case, fr, g, level, marks, X, tau=0.0):
    """engine.explain_hop / texplain_hop / xexplain_hop as numpy: .edges int64 [E, 4], .alpha float32, .time int64 or None, .heads."""
    from red_gnn_amd import engine as eng
    fn = {"static": eng.explain_hop, "temporal": eng.texplain_hop, "windowed": eng.xexplain_hop}[case.kind]
    out = fn(fr, g, level, _marks_dev(marks), *(X[k] for k in ATTN), case.attn_dim, tau)
    torch.cuda.synchronize()
    return types.SimpleNamespace(heads=_marks_np(out[0]), edges=out[1].cpu().numpy().astype(np.int64), alpha=out[2].cpu().numpy(),
                                 time=out[3].cpu().numpy().astype(np.int64) if len(out) > 3 else None)


def _count(case, fr, g, level, marks, X, tau):
    """The count pass alone: (head marks, word pointer int32 [B * W + 1] pre-filled with -1, the host's edge count)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    m = _marks_dev(marks)
    heads = torch.full_like(m, -1)
    word_ptr = torch.full((m.numel() + 1,), -1, dtype=torch.int32, device="cuda")
    nb = L.rg_explain_scratch_bytes(fr.handle)
    scratch = torch.empty(nb + 256, dtype=torch.uint8, device="cuda")
    aligned = (scratch.data_ptr() + 255) // 256 * 256
    n_e = C.c_int64(-1)
    _lib.check(getattr(L, ENTRY[case.kind] + "_count")(
        fr.handle, g.handle, case.B, case.n_ent, level, p(m), p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), case.ap, p(X["w_alpha"]), p(X["b_alpha"]),
        case.attn_dim, float(tau), p(heads), p(word_ptr), C.c_void_p(aligned), nb, C.byref(n_e), _lib.stream_ptr()))
    torch.cuda.synchronize()
    return _marks_np(heads), word_ptr.cpu().numpy().astype(np.int64), n_e.value


def graph_export(case, g):
    in_ptr, in_hr = g.export()[2:]
    return in_ptr, in_hr, (None if case.kind == "static" else g.export_time()[1])


def same(tag, got, exp, alpha=True):
    """A device hop result against hop_ref.select_edges' namespace: edges in order, head marks word for word, time ids, alpha bits."""
    assert got.edges.shape == exp.edges.shape, "%s: %d edges, the reference has %d" % (tag, len(got.edges), len(exp.edges))
    assert np.array_equal(got.edges, exp.edges), "%s: edges differ, first at %s" % (tag, np.argwhere(got.edges != exp.edges)[:1])
    assert np.array_equal(got.heads, exp.heads), "%s: %d words of the head marks differ" % (tag, int((got.heads != exp.heads).sum()))
    if exp.time is not None:
        assert np.array_equal(got.time, exp.time), tag + ": time ids / data rows"
    if alpha and exp.alpha is not None:
        assert np.array_equal(got.alpha.view(np.uint32), exp.alpha.view(np.uint32)), tag + ": alpha bits"


def walk(name, then=None):
    """Generator over a case's hops: expands the frontier, checks its node list, yields a record per hop while the frontier stands at
    that level.  After the last hop it calls ``then`` (the graph still open), then closes the frontier and the graph."""
    case = hr.CASES[name]()
    g, fr = _setup(case)
    ex = _extra(case)
    gx = graph_export(case, g)
    try:
        for k, (old, new, edges, hop) in enumerate(lr.hops(case)):
            tag = "%s hop %d" % (name, k + 1)
            n_new, n_e, n_old = fr.expand(g)
            nodes, _, _ = fr.nodes()
            assert (n_old, n_e) == (hop.n_old, hop.E), tag
            assert np.array_equal(nodes.cpu().numpy().astype(np.int64), new), tag + ": frontier nodes differ from the oracle's"
            x = lr.inputs(case, k, hop)
            yield types.SimpleNamespace(case=case, g=g, fr=fr, ex=ex, gx=gx, k=k, level=k + 1, tag=tag, old=old, new=new, edges=edges, hop=hop,
                                        x=x, X={kk: _dev(v) for kk, v in x.items()}, nodes=nodes,
                                        full=hr.bitmap(new, case.B, case.n_ent))
        if then is not None:
            then()
    finally:
        fr.close()
        g.close()


def device_alphas(h):
    """Step 1's call: every node of the level marked, tau = 0.  Returns (result, hop_ref candidates, AlphaTable of the device's alphas)."""
    got = explain(h.case, h.fr, h.g, h.level, h.full, h.X, 0.0)
    cands = hr.hop_candidates(h.case, h.gx, h.old, h.full)
    same(h.tag + " all marked", got, hr.select_edges(cands))      # (the edges first: the table below needs every one of them)
    tab = hr.AlphaTable(h.case.n_ent, h.case.n_rela_rows, got.edges[:, 0], got.edges[:, 1], got.edges[:, 2], got.alpha)
    return got, cands, tab


def _patterns(h, rng):
    """Step 4's marks: (name, uint32 [B, W]) pairs.  Never a bit at an entity >= n_ent."""
    case, new = h.case, h.new
    B, n_ent, W = case.B, case.n_ent, hr.n_words(case.n_ent)
    bm = lambda nodes: hr.bitmap(nodes, B, n_ent)
    first = np.flatnonzero(np.diff(new[:, 0], prepend=-1))                   # the rows' first node
    size = np.diff(np.append(first, len(new)))
    yield "no mark", np.zeros((B, W), np.uint32)
    yield "one node per row", bm(new[first + rng.integers(0, size)])
    yield "half of the level", bm(new[rng.random(len(new)) < 0.5])
    yield "bits 0 and 31", bm(new[np.isin(new[:, 1] & 31, (0, 31))])
    yield "first word", bm(new[new[:, 1] < 32])
    yield "last word", bm(new[new[:, 1] >= 32 * (W - 1)])
    # one row's entities outside its level: the neighbours of its nodes' ids and both ends of the id range
    in_level = h.full
    for b in sorted({int(new[0, 0]), int(new[-1, 0])}):
        mine = new[new[:, 0] == b, 1]
        cand = np.unique(np.clip(np.concatenate([mine[:40] + 1, mine[:40] - 1, [0, 31, 32, n_ent - 1, 32 * (W - 1)]]), 0, n_ent - 1))
        cand = cand[((in_level[b, cand >> 5] >> (cand & 31).astype(np.uint32)) & 1) == 0]
        if len(cand):
            yield "row %d outside its level" % b, bm(np.stack([np.full(len(cand), b), cand], 1))


def _bits_of(agg, rows, cols):
    return np.ascontiguousarray(agg[rows, cols]).view(np.uint32)


@pytest.mark.parametrize("name", list(hr.CASES))
def test_explain_hop_vs_reference(name, monkeypatch):
    from red_gnn_amd import _lib, engine as eng
    t0 = time.time()
    rng = np.random.default_rng(7)
    emits = []
    L = _lib.lib()
    for entry in ENTRY.values():      # count the emit launches (step 5: none where the count pass found no edge)
        fn = getattr(L, entry + "_emit")
        monkeypatch.setattr(L, entry + "_emit", lambda *a, _fn=fn: (emits.append(1), _fn(*a))[1])
    records = []

    def after():      # ---- 7. gather, 8. rows alone
        _gather(records, rng)
        if name in hr.SMALL:
            _rows_alone(records, rng)
    for h in walk(name, after):
        case, tag = h.case, h.tag
        # ---- 1. everything marked, tau = 0
        got, cands, tab = device_alphas(h)
        exp = hr.select_edges(cands, tab, 0.0)
        same(tag + " all marked", got, exp)
        assert len(got.edges) == h.hop.E and got.alpha.dtype == np.float32, tag
        old_idx = np.searchsorted(h.old[:, 0] * case.n_ent + h.old[:, 1], got.edges[:, 0] * case.n_ent + got.edges[:, 1])
        rows = lambda *cols: np.stack(cols, 1)[np.lexsort(cols[::-1])]
        if case.kind == "static":
            assert np.array_equal(rows(*got.edges.T, old_idx), rows(*h.edges[:, :5].T)), tag + ": not the oracle's hop"
        else:      # (the time field through what the layers read of it: direction and time-table row)
            mine = lr.hop_of(case, np.column_stack([got.edges, old_idx, old_idx]), got.time, len(h.old), len(h.new))
            tf = (lambda o: o.dir) if case.kind == "temporal" else (lambda o: o.trow)
            assert np.array_equal(rows(*got.edges.T, old_idx, tf(mine), mine.trow), rows(*h.edges[:, :5].T, tf(h.hop), h.hop.trow)), tag
        heads, word_ptr, n_e = _count(case, h.fr, h.g, h.level, h.full, h.X, 0.0)
        assert np.array_equal(heads, exp.heads) and n_e == h.hop.E, tag
        assert word_ptr[0] == 0 and word_ptr[-1] == h.hop.E and (np.diff(word_ptr) >= 0).all(), tag + ": word pointer"
        assert np.array_equal(np.diff(word_ptr), exp.word_count), tag + ": edges per word"

        # ---- 2. alpha against fp64
        a64, kap, bnd = hr.alpha_ref(case, h.hop, h.x)
        ref = {kk: hr.AlphaTable(case.n_ent, case.n_rela_rows, h.edges[:, 0], h.edges[:, 1], h.edges[:, 2], v).at(*got.edges[:, :3].T)
               for kk, v in (("a", a64), ("k", kap), ("b", bnd))}
        ratio = hr.alpha_ratio(got.alpha, ref["a"], ref["k"], case)
        err = np.abs(got.alpha.astype(np.float64) - ref["a"])
        print("%s (E %d): alpha worst ratio %.3g (allowed %.3g), largest |error| %.3g" % (tag, len(err), ratio, lr.C_BOUND, err.max(initial=0)))
        assert (err <= ref["b"]).all(), "%s: %d alphas beyond the bound, worst ratio %.3g" % (tag, int((err > ref["b"]).sum()), ratio)

        # ---- 3. alpha against the forward, bit for bit (one-hot readout)
        Y = {kk: _dev(v) for kk, v in hr.one_hot_tables(case, h.x).items()}
        if case.kind == "static":
            agg = eng.layer_fwd(h.fr, h.g, h.level, h.nodes, Y["hidden"], Y["rela"], case.d, Y["a_s"], Y["a_r"], Y["a_q"], Y["w_alpha"],
                                Y["b_alpha"], case.attn_dim)
        else:
            agg = _forward(case, h.g, h.fr, Y, h.ex, len(h.new), 1)
        agg = agg.cpu().numpy()
        new_idx = np.searchsorted(h.new[:, 0] * case.n_ent + h.new[:, 1], got.edges[:, 0] * case.n_ent + got.edges[:, 3])
        single = hr.singleton_mask(types.SimpleNamespace(o=new_idx, r=got.edges[:, 2]), case.d)
        assert single.mean() >= 0.5, tag
        fwd = _bits_of(agg, new_idx[single], got.edges[single, 2] % case.d)
        mine = got.alpha[single].view(np.uint32)
        assert np.array_equal(fwd, mine), ("%s: %d of %d singleton edges differ from the forward's alpha bits; first: explain %r forward %r"
                                           % (tag, int((fwd != mine).sum()), len(mine), mine[fwd != mine][:1].view(np.float32),
                                              fwd[fwd != mine][:1].view(np.float32)))

        # ---- 4. mark patterns at tau = 0 and at an alpha that occurs
        a_star = np.sort(got.alpha)[len(got.alpha) // 2]
        for what, marks in _patterns(h, rng):
            c = cands if marks is h.full else hr.hop_candidates(case, h.gx, h.old, marks)
            for tau in (0.0, float(a_star)):
                same("%s %s tau %.9g" % (tag, what, tau), explain(case, h.fr, h.g, h.level, marks, h.X, tau), hr.select_edges(c, tab, tau))
            if what == "no mark" or "outside" in what:
                assert len(hr.select_edges(c, tab, 0.0).edges) == 0, tag + " " + what

        # ---- 5. the >= edge
        up = np.nextafter(a_star, np.float32(np.inf))
        keep, drop = (explain(case, h.fr, h.g, h.level, h.full, h.X, float(t)) for t in (a_star, up))
        same(tag + " tau = a*", keep, hr.select_edges(cands, tab, a_star))
        same(tag + " tau = nextafter(a*)", drop, hr.select_edges(cands, tab, up))
        n_eq = int((got.alpha == a_star).sum())
        assert n_eq >= 1 and len(keep.edges) - len(drop.edges) == n_eq and (keep.alpha >= a_star).all() and (drop.alpha > a_star).all(), tag
        assert len(keep.edges) == int((got.alpha >= a_star).sum()), tag
        del emits[:]
        none = explain(case, h.fr, h.g, h.level, h.full, h.X, float("inf"))
        assert len(none.edges) == 0 and not none.heads.any() and not emits, tag + ": tau = +inf"
        same(tag + " tau = -inf", explain(case, h.fr, h.g, h.level, h.full, h.X, float("-inf")), exp)
        assert len(emits) == 1, tag

        # ---- 6. seed
        _seed(h, rng)

        # ---- 8. two runs are bitwise equal
        same(tag + " second run", explain(case, h.fr, h.g, h.level, h.full, h.X, 0.0), got)
        records.append(types.SimpleNamespace(h=h, got=got, a_star=float(a_star)))

    print("%s: %.2f s" % (name, time.time() - t0))


def _seed(h, rng):
    """rg_explain_seed: per row an object inside the level (its last node or a random one), a valid entity outside it, -1 or n_ent; the
    kinds rotate over the rows in four calls, so every row sees every kind."""
    from red_gnn_amd import engine as eng
    case, new = h.case, h.new
    B, n_ent, W = case.B, case.n_ent, hr.n_words(case.n_ent)
    first = np.flatnonzero(np.diff(new[:, 0], prepend=-1))
    size = np.diff(np.append(first, len(new)))
    has = np.zeros(B, bool)
    has[new[first, 0]] = True
    inside = np.full(B, -1, np.int64)
    pick = np.where(rng.random(len(first)) < 0.5, size - 1, rng.integers(0, size))
    inside[new[first, 0]] = new[first + pick, 1]
    outside = np.full(B, -1, np.int64)
    for b in range(B):      # the first entity from a random start that is not in the row's level (a row's level never holds every entity twice)
        for e in (int(rng.integers(0, n_ent)), n_ent - 1, 0, 1, 2):
            if not (h.full[b, e >> 5] >> np.uint32(e & 31)) & 1:
                outside[b] = e
                break
    for shift in range(4):
        kind = (np.arange(B) + shift) % 4
        objs = np.select([kind == 0, kind == 1, kind == 2], [inside, outside, np.full(B, -1)], n_ent)
        reached = (kind == 0) & has
        want = hr.bitmap(np.stack([np.arange(B), objs], 1)[reached], B, n_ent)
        marks, got = eng.explain_seed(h.fr, h.level, _dev(objs, torch.int32))
        assert np.array_equal(got.cpu().numpy(), reached), h.tag + ": seed reached"
        assert np.array_equal(_marks_np(marks), want), h.tag + ": seed marks"


def _gather(records, rng):
    """rg_explain_gather: the hops' lists into one (row, hop, head, rel, tail) array - rows' blocks in a shuffled order, a row's hops in
    order - against the same placement in numpy.  The median-tau lists, so that rows lose different numbers of edges."""
    from red_gnn_amd import engine as eng
    case = records[0].h.case
    B = case.B
    lists = []
    for r in records:
        keep = r.got.alpha >= np.float32(r.a_star)
        lists.append((r.got.edges[keep], r.got.alpha[keep]))
    counts = np.stack([np.bincount(e[:, 0], minlength=B) for e, _ in lists])          # [L, B]
    order = rng.permutation(B)
    per_row = counts.sum(0)
    offsets = np.zeros(B, np.int64)
    offsets[order] = np.cumsum(per_row[order]) - per_row[order]
    n_out = int(per_row.sum()) + 3                                                     # three rows past the lists stay untouched
    want_e, want_a = np.full((n_out, 5), -7, np.int64), np.full(n_out, -7.0, np.float32)
    out_e = torch.full((n_out, 5), -7, dtype=torch.int32, device="cuda")
    out_a = torch.full((n_out,), -7.0, dtype=torch.float32, device="cuda")
    before = np.cumsum(counts, 0) - counts
    for l, (e, al) in enumerate(lists, 1):
        row_first = np.cumsum(counts[l - 1]) - counts[l - 1]
        row_base = offsets + before[l - 1]
        dst = row_base[e[:, 0]] + np.arange(len(e)) - row_first[e[:, 0]]
        want_e[dst] = np.column_stack([e[:, 0], np.full(len(e), l), e[:, 1:]])
        want_a[dst] = al
        dev_e = _dev(e, torch.int32) if len(e) else torch.empty((0, 4), dtype=torch.int32, device="cuda")
        eng.explain_gather(l, B, dev_e, _dev(al), _dev(row_first, torch.int64), _dev(row_base, torch.int64), out_e, out_a)
    empty = torch.empty((0, 4), dtype=torch.int32, device="cuda")                     # n = 0: a no-op
    eng.explain_gather(1, B, empty, torch.empty(0, device="cuda"), _dev(np.zeros(B), torch.int64), _dev(np.zeros(B), torch.int64), out_e, out_a)
    torch.cuda.synchronize()
    assert np.array_equal(out_e.cpu().numpy(), want_e), case.name + ": gathered edges"
    assert np.array_equal(out_a.cpu().numpy().view(np.uint32), want_a.view(np.uint32)), case.name + ": gathered alpha"
    assert (want_e[:-3, 0] >= 0).all() and (want_e[-3:] == -7).all()


def sub_batch(case, rows):
    """The case restricted to the queries ``rows`` (in that order, renamed 0, 1, ..) and its frontier at level 0.  The levels of a query
    do not depend on the others, so the level-l node list of the result is the rows' slices of the whole batch's, in that order."""
    from red_gnn_amd import engine as eng
    rows = np.asarray(rows, np.int64)
    one = types.SimpleNamespace(**vars(case))
    one.B, one.reset = len(rows), "nodes"
    one.nodes0 = np.concatenate([np.column_stack([np.full(int((case.nodes0[:, 0] == b).sum()), i), case.nodes0[case.nodes0[:, 0] == b, 1]])
                                 for i, b in enumerate(rows)], 0)
    for k in ("q_time", "win_lo", "win_hi", "loop_time"):
        if hasattr(case, k):
            setattr(one, k, np.asarray(getattr(case, k))[rows])
    fr = eng.Frontier(case.n_ent, one.B, n_levels=case.hops + 1)
    if case.kind == "windowed":
        fr.set_window(_dev(one.win_lo, torch.int32), _dev(one.win_hi, torch.int32), case.n_data)
    fr.reset_nodes(_dev(one.nodes0, torch.int32))
    return one, fr


def sub_tables(h, rows):
    """The hop's device tables for sub_batch(case, rows): the rows' slices of a_s in that order, their a_q rows."""
    idx = np.concatenate([np.flatnonzero(h.old[:, 0] == b) for b in rows])
    return dict(h.X, a_s=h.X["a_s"][torch.as_tensor(idx).cuda()].contiguous(),
                a_q=h.X["a_q"][torch.as_tensor(np.asarray(rows, np.int64)).cuda()].contiguous())


def _rows_alone(records, rng):
    """A batch row taken alone - a frontier of B = 1 from the row's start, its slice of a_s, its a_q row, its window - gives the row's
    slice of the batch's edges (row renamed 0), alpha bits, time ids and head marks, at tau = 0 and at the median."""
    case = records[0].h.case
    g, n_ent = records[0].h.g, case.n_ent
    for b in sorted({0, case.B - 1, int(rng.integers(0, case.B))}):
        one, fr = sub_batch(case, [b])
        for r in records:
            h = r.h
            fr.expand(g)
            X = sub_tables(h, [b])
            assert fr.n_old == X["a_s"].shape[0], h.tag
            for tau in (0.0, r.a_star):
                got = explain(one, fr, g, h.level, h.full[b:b + 1], X, tau)
                sel = (r.got.edges[:, 0] == b) & (r.got.alpha >= np.float32(tau))
                want = r.got.edges[sel].copy()
                want[:, 0] = 0
                whole_heads = hr.bitmap(r.got.edges[sel][:, :2], case.B, n_ent)[b:b + 1]
                same("%s row %d alone tau %.9g" % (h.tag, b, tau), got, types.SimpleNamespace(
                    edges=want, heads=whole_heads, alpha=r.got.alpha[sel], time=None if r.got.time is None else r.got.time[sel]))
        fr.close()
