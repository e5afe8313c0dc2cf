"""T_RED_GNN.explain on the MI355X (-m gpu): the r-digraph of (head, relation, time, o) with the attention and the time id of every
edge, against the float64 reference walk (tests/temporal_ref.py), and its properties.  Tolerances: alpha as tests/test_explain_gpu.py
(RTOL, ATOL = 1e-4, 1e-5); scores as test_temporal_per_layer_tables_vs_oracle (RTOL, ATOL_H = 1e-4, 5e-5); integers exact."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests import explain_ref as X
from tests import layer_ref as LR
from tests import temporal_ref as TR

pytestmark = pytest.mark.gpu

RTOL, ATOL, ATOL_H = 1e-4, 1e-5, 5e-5


def _rows(last, n_q, n_ent, rng, per_query=3, extra=1):
    """(query index, answer) rows: per_query entities of each query's last level and `extra` outside it."""
    q_of, objs = [], []
    for q in range(n_q):
        inside = last[last[:, 0] == q, 1]
        pick = rng.choice(inside, min(per_query, len(inside)), replace=False)
        outside = np.setdiff1d(np.arange(n_ent), inside)
        out = rng.choice(outside, min(extra, len(outside)), replace=False) if len(outside) else []
        for o in list(pick) + list(out):
            q_of.append(q)
            objs.append(int(o))
    return np.array(q_of), np.array(objs)


def _last_level_answers(model, B):
    """Per query the last entity of its last level in the forward that just ran (model.last_nodes)."""
    nodes = model.last_nodes.cpu().numpy()
    return np.array([nodes[nodes[:, 0] == b][-1, 1] for b in range(B)])


def _check(rd, exp, q_time_rows, what=""):
    edges, time, alpha, offsets, reached = exp
    got = rd.edges.cpu().numpy()
    assert got.shape == edges.shape, (what, got.shape, edges.shape)
    assert np.array_equal(got, edges), what
    assert rd.time.dtype == torch.int32 and np.array_equal(rd.time.cpu().numpy(), time), what
    assert np.array_equal(rd.offsets.cpu().numpy(), offsets), what
    assert np.array_equal(rd.reached.cpu().numpy(), reached), what
    assert rd.q_time.dtype == torch.int32 and np.array_equal(rd.q_time.cpu().numpy(), q_time_rows), what
    np.testing.assert_allclose(rd.alpha.cpu().numpy(), alpha, rtol=RTOL, atol=ATOL, err_msg=what)
    assert np.array_equal(rd.direction().cpu().numpy(), TR.direction(time, np.asarray(q_time_rows)[edges[:, 0]])), what


def _case(model, quads, n_ent, heads, rels, times, q_of, objs, n_layer, act, shared, taus=(0.3, 0.6)):
    """explain against the walk at tau = 0; tau > 0 is applied to the device's own tau = 0 alphas (same edges, same order), so that
    alphas within rounding of tau cannot flip the comparison."""
    scores, hops, last = TR.walk(TR.state_of(model), quads, n_ent, heads, rels, times, n_layer, act, shared_tables=shared)
    batch = {"head": heads[q_of], "relation": rels[q_of], "time": times[q_of]}
    rd0 = model.explain(batch, objs)
    _check(rd0, TR.expected_digraph(hops, q_of, objs, last, 0.0, n_ent, model.graph), times[q_of], "tau=0")
    ref_score = scores[q_of, objs]
    np.testing.assert_allclose(rd0.score.cpu().numpy(), ref_score, rtol=RTOL, atol=ATOL_H)
    e0, a0, t0 = rd0.edges.cpu().numpy(), rd0.alpha.cpu().numpy(), rd0.time.cpu().numpy()
    for tau in taus:
        ok = X.rdigraph_mask(e0[:, 0], e0[:, 1], e0[:, 2], e0[:, 4], a0, objs, rd0.reached.cpu().numpy(), tau, n_ent, n_layer)
        rd = model.explain(batch, objs, min_alpha=tau)
        assert np.array_equal(rd.edges.cpu().numpy(), e0[ok]), tau
        assert np.array_equal(rd.time.cpu().numpy(), t0[ok]), tau
        assert np.array_equal(rd.alpha.cpu().numpy(), a0[ok]), tau
        assert (rd.alpha.cpu().numpy() >= tau).all()
        assert np.array_equal(rd.offsets.cpu().numpy()[1:], np.cumsum(np.bincount(e0[ok][:, 0], minlength=len(q_of))))
    return rd0, hops, last


@pytest.mark.parametrize("d,a,act,n_layer,shared,B,m", [(16, 3, "idd", 2, False, 33, 1500), (20, 5, "tanh", 3, True, 9, 600),
                                                      (32, 30, "relu", 4, False, 5, 300), (64, 5, "relu", 3, False, 9, 600),
                                                      (16, 3, "tanh", 2, True, 5, 600)])
def test_explain_vs_walk_widths_depths_layouts(d, a, act, n_layer, shared, B, m):
    """layer_ref._temporal_case: 200 entities (7 bitmap words, the last partly used; B * 7 is no multiple of 64), 12 time ids, query
    times 0, n_time - 1 and n_time / 2 (equal to edge times), hub tails, duplicated facts."""
    c = LR._temporal_case("explain", seed=n_layer, B=B, m=m)
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, n_layer, d, a, act, shared=shared)
    heads, rels = c.nodes0[:, 1], (np.arange(B) * 3) % c.n_rela_rows
    _, _, last = TR.walk(TR.state_of(model), c.quads, c.n_ent, heads, rels, c.q_time, n_layer, act, shared_tables=shared)
    q_of, objs = _rows(last, B, c.n_ent, np.random.default_rng(0), per_query=2 if B > 9 else 3)
    assert (B * ((c.n_ent + 31) // 32)) % 64 != 0 and c.n_ent % 32 != 0
    _case(model, c.quads, c.n_ent, heads, rels, c.q_time, q_of, objs, n_layer, act, shared)


def _hand(n_layer=2, d=32, a=5, act="relu"):
    quads = TR.hand_graph()
    model = TR.make_model(quads, TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1, TR.HAND_N_TIME, n_layer, d, a, act)
    # queries: the three hubs (times 0 and n_time - 1 among them), leaf 3 at time 5 twice (between the two times of its repeated
    # fact), the isolated entity, and 260 at time 4 (the time of its edge to 70)
    heads = np.array([0, 1, 2, 3, 299, 260])
    rels = np.array([0, 1, 2, 6, 4, 1])
    times = np.array([0, TR.HAND_N_TIME - 1, 5, 5, 3, 4])
    return quads, model, heads, rels, times


def test_hand_graph_degrees_repeated_fact_and_rows():
    """Tails of in-degree 1 / 64 / 65 / 129 (one lane, a full 64-lane step, a step and one lane, two steps and one lane), the fact
    (3, 0, 0) at times 2 and 8 around the query time 5 with an exact duplicate, a row whose o is outside level L, one query in two rows
    with different o; 7 rows x 10 words = 70 mark words (no multiple of 64)."""
    quads, model, heads, rels, times = _hand()
    q_of = np.array([0, 1, 2, 3, 3, 4, 5])
    objs = np.array([0, 1, 2, 0, 3, 299, 5])
    rd, hops, last = _case(model, quads, TR.HAND_N_ENT, heads, rels, times, q_of, objs, 2, "relu", False)
    reached = rd.reached.cpu().numpy()
    assert reached.tolist() == [True] * 6 + [False]
    e, t, off = rd.edges.cpu().numpy(), rd.time.cpu().numpy(), rd.offsets.cpu().numpy()
    assert off[7] == off[6]                                              # the unreached row has no edges
    # hub rows: at hop 2 every in-edge of the hub is kept (its leaves are all in level 1)
    for row, deg in ((0, 64), (1, 65), (2, 129)):
        assert ((e[:, 0] == row) & (e[:, 1] == 2) & (e[:, 4] == row)).sum() == deg
    assert ((e[:, 0] == 5) & (e[:, 1] == 2)).sum() == 1                  # entity 299: the identity edge alone
    # row 3 = (3, r, time 5) -> 0: the fact (3, 0, 0) once per quadruple at hop 1, in CSR (fact-row) order: time 2, 8, 2
    m = (e[:, 0] == 3) & (e[:, 1] == 1) & (e[:, 2] == 3) & (e[:, 3] == 0) & (e[:, 4] == 0)
    assert t[m].tolist() == [2, 8, 2]
    assert rd.direction().cpu().numpy()[m].tolist() == [0, 2, 0]
    al = rd.alpha.cpu().numpy()[m]
    assert al[0] == al[1] == al[2]                                       # the attention does not read the time
    # the same query in rows 3 and 4: different digraphs of one subgraph
    assert not np.array_equal(e[off[3]:off[4], 1:], e[off[4]:off[5], 1:])


def test_argmax_batch_invariance_determinism_training_flag():
    quads, model, heads, rels, times = _hand()
    batch = {"head": heads, "relation": rels, "time": times}
    with torch.no_grad():
        s = model(batch, mode="test")
    rd_top = model.explain(batch)
    rd_arg = model.explain(batch, s.argmax(1).cpu().numpy())
    fields = ("edges", "alpha", "time", "offsets", "reached", "score", "q_time")
    for f in fields:
        assert torch.equal(getattr(rd_top, f), getattr(rd_arg, f)), f
    assert torch.equal(rd_top.score, s.max(1).values)
    objs = np.array([0, 1, 2, 0, 299, 70])
    rd = model.explain(batch, objs)
    rd2 = model.explain(batch, objs)
    for f in fields:
        assert torch.equal(getattr(rd, f), getattr(rd2, f)), f
    off = rd.offsets.cpu().numpy()
    assert rd.reached.all()
    for b in range(len(heads)):
        one = model.explain({k: v[b:b + 1] for k, v in batch.items()}, objs[b:b + 1])
        sl = slice(off[b], off[b + 1])
        e = rd.edges[sl].clone()
        e[:, 0] = 0
        assert torch.equal(one.edges, e) and torch.equal(one.time, rd.time[sl]) and torch.equal(one.alpha, rd.alpha[sl]), b
    model.dropout.p = 0.5
    model.train()
    rd3 = model.explain(batch, objs)
    assert model.training
    model.eval()
    for f in ("edges", "alpha", "time", "offsets", "reached"):
        assert torch.equal(getattr(rd, f), getattr(rd3, f)), f


@pytest.mark.parametrize("d,a,act,n_layer", [(64, 30, "relu", 3), (20, 5, "tanh", 2)])
def test_faithfulness_model_on_the_digraph_alone(d, a, act, n_layer):
    """A second T_RED_GNN with the same weights whose graph holds only the digraph's quadruples scores o like the full model."""
    c = LR._temporal_case("faith", seed=21, B=4, m=500)
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, n_layer, d, a, act)
    heads, rels = c.nodes0[:, 1], np.array([0, 3, 7, 10])
    batch = {"head": heads, "relation": rels, "time": c.q_time}
    with torch.no_grad():
        full = model(batch, mode="test").cpu().numpy()
    objs = _last_level_answers(model, 4)
    rd = model.explain(batch, objs)
    assert rd.reached.all()
    e, t, off = rd.edges.cpu().numpy(), rd.time.cpu().numpy(), rd.offsets.cpu().numpy()
    for b in range(4):
        sl = slice(off[b], off[b + 1])
        sub_quads = np.unique(np.column_stack([e[sl, 2:5], t[sl]]), axis=0)
        sub = TR.make_model(sub_quads, c.n_ent, c.n_rela_rows, c.n_time, n_layer, d, a, act, state=model.state_dict())
        with torch.no_grad():
            got = sub({k: v[b:b + 1] for k, v in batch.items()}, mode="test")[0, objs[b]].item()
        ref = full[b, objs[b]]
        print("row %d: %d quadruples of %d, score %.6g vs %.6g" % (b, len(sub_quads), len(c.quads), got, ref))
        assert ref != 0.0 and abs(got - ref) <= RTOL * abs(ref) + ATOL_H, (b, got, ref)


@pytest.mark.parametrize("n_layer", [2, 3])
def test_strongest_paths_against_brute_force(n_layer):
    c = LR._temporal_case("paths", seed=3, B=6, m=400)
    model = TR.make_model(c.quads, c.n_ent, c.n_rela_rows, c.n_time, n_layer, 32, 5, "relu")
    heads, rels = c.nodes0[:, 1], np.arange(6) % c.n_rela_rows
    batch = {"head": heads, "relation": rels, "time": c.q_time}
    with torch.no_grad():
        model(batch, mode="test")
    rd = model.explain(batch, _last_level_answers(model, 6))
    assert rd.reached.all()
    rl, en, pr = (x.cpu().numpy() for x in rd.strongest_paths())
    e, al, off = rd.edges.cpu().numpy(), rd.alpha.cpu().numpy().astype(np.float64), rd.offsets.cpu().numpy()
    for b in range(6):
        rows = np.arange(off[b], off[b + 1])
        if len(rows) == 0:
            assert (en[b] == -1).all() and pr[b] == 0.0
            continue
        by_hop = [rows[e[rows, 1] == l] for l in range(1, n_layer + 1)]
        best = 0.0
        for path in itertools.product(*by_hop):
            if e[path[0], 2] != heads[b] or any(e[path[i], 4] != e[path[i + 1], 2] for i in range(n_layer - 1)):
                continue
            prod = 1.0
            for i in path:
                prod *= al[i]
            best = max(best, prod)
        assert best > 0 and pr[b] == best, (b, pr[b], best)
        assert en[b, 0] == heads[b] and en[b, -1] == e[rows[-1], 4]


def test_ids_are_validated():
    quads, model, heads, rels, times = _hand()
    ok = {"head": [0], "relation": [0], "time": [0]}
    for bad in ({"head": [TR.HAND_N_ENT]}, {"relation": [2 * TR.HAND_N_REL + 1]}, {"time": [TR.HAND_N_TIME]}, {"head": [-1]},
                {"head": [0, 1]}, {"head": [], "relation": [], "time": []}):
        with pytest.raises(ValueError):
            model.explain({**ok, **bad}, None)
    with pytest.raises(ValueError):
        model.explain(ok, [TR.HAND_N_ENT])
    with pytest.raises(ValueError):
        model.explain(ok, [0, 1])
    with pytest.raises(ValueError):
        model.explain(ok, [0], min_alpha=float("nan"))
    assert model.explain(ok, [0]).reached.all()


def test_argument_errors():
    """Argument errors return non-zero with a message before any device work."""
    from red_gnn_amd import _lib, engine
    quads = TR.hand_graph()
    n_ent, R = TR.HAND_N_ENT, 2 * TR.HAND_N_REL + 1
    tg = engine.TemporalGraph(n_ent, R, TR.HAND_N_TIME, quads)
    sg = engine.Graph(n_ent, TR.HAND_N_REL, quads[:100, :3])
    L = _lib.lib()
    s = _lib.stream_ptr()

    def frontier(graph, window=False):
        fr = engine.Frontier(n_ent, 4, 3)
        fr.reset(torch.zeros(4, dtype=torch.int32, device="cuda"))
        fr.expand(graph)
        if window:                                                       # (set after the hop: only the entry points' check sees it)
            z = torch.zeros(4, dtype=torch.int32, device="cuda")
            fr.set_window(z, z + 5, 10)
        return fr
    W = (n_ent + 31) // 32
    marks = torch.zeros((4, W), dtype=torch.int32, device="cuda")
    prev = torch.zeros_like(marks)
    wp = torch.zeros(marks.numel() + 1, dtype=torch.int32, device="cuda")
    f32 = torch.zeros((max(R, 4), 4), dtype=torch.float32, device="cuda")
    n_e = C.c_int64()
    fr_t, fr_s, fr_w = frontier(tg), frontier(sg), frontier(tg, window=True)
    scr = torch.zeros(L.rg_explain_scratch_bytes(fr_t.handle) + 512, dtype=torch.uint8, device="cuda")
    scr_p = (scr.data_ptr() + 255) // 256 * 256
    scr_n = scr.numel() - (scr_p - scr.data_ptr())

    def count(fn, fr, g, marks_p=_lib.ptr(marks), prev_p=_lib.ptr(prev), level=1):
        return fn(fr.handle, g.handle, 4, n_ent, level, marks_p, _lib.ptr(f32), _lib.ptr(f32), _lib.ptr(f32), 4, _lib.ptr(f32),
                  _lib.ptr(f32), 3, 0.0, prev_p, _lib.ptr(wp), C.c_void_p(scr_p), scr_n, C.byref(n_e), s)

    def emit(fr, g, edges_p, alpha_p, time_p):
        return L.rg_texplain_emit(fr.handle, g.handle, 4, n_ent, 1, _lib.ptr(marks), _lib.ptr(f32), _lib.ptr(f32), _lib.ptr(f32), 4,
                                  _lib.ptr(f32), _lib.ptr(f32), 3, 0.0, _lib.ptr(wp), edges_p, alpha_p, time_p, s)
    assert count(L.rg_texplain_count, fr_s, sg) != 0 and b"temporal graphs only" in L.rg_last_error()
    assert count(L.rg_texplain_count, fr_w, tg) != 0 and b"window" in L.rg_last_error()
    assert count(L.rg_explain_count, fr_t, tg) != 0 and b"static graphs only" in L.rg_last_error()
    assert count(L.rg_texplain_count, fr_t, tg, marks_p=None) != 0 and b"NULL" in L.rg_last_error()
    assert count(L.rg_texplain_count, fr_t, tg, prev_p=None) != 0 and b"NULL" in L.rg_last_error()
    assert count(L.rg_texplain_count, fr_t, tg, level=2) != 0 and b"not resident" in L.rg_last_error()
    assert L.rg_texplain_count(None, tg.handle, 4, n_ent, 1, _lib.ptr(marks), _lib.ptr(f32), _lib.ptr(f32), _lib.ptr(f32), 4, _lib.ptr(f32),
                               _lib.ptr(f32), 3, 0.0, _lib.ptr(prev), _lib.ptr(wp), C.c_void_p(scr_p), scr_n, C.byref(n_e), s) != 0
    assert b"NULL" in L.rg_last_error()
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    al = torch.zeros(16, dtype=torch.float32, device="cuda")
    tm = torch.zeros(16, dtype=torch.int32, device="cuda")
    assert emit(fr_t, tg, _lib.ptr(buf), _lib.ptr(al), None) != 0 and b"NULL" in L.rg_last_error()
    assert emit(fr_t, tg, None, _lib.ptr(al), _lib.ptr(tm)) != 0 and b"NULL" in L.rg_last_error()
    assert emit(fr_t, tg, C.c_void_p(buf.data_ptr() + 4), _lib.ptr(al), _lib.ptr(tm)) != 0 and b"16-B aligned" in L.rg_last_error()
    assert emit(fr_s, sg, _lib.ptr(buf), _lib.ptr(al), _lib.ptr(tm)) != 0 and b"temporal graphs only" in L.rg_last_error()
    assert emit(fr_w, tg, _lib.ptr(buf), _lib.ptr(al), _lib.ptr(tm)) != 0 and b"window" in L.rg_last_error()
    # export_time: a static graph has no times; a temporal one returns them beside export()'s entries
    with pytest.raises(_lib.NativeError):
        engine.TemporalGraph.export_time(sg)
    ot, it = tg.export_time()
    op, ort, ip, ihr = tg.export()
    got = sorted(zip(ihr[:, 0].tolist(), ihr[:, 1].tolist(), np.repeat(np.arange(n_ent), np.diff(ip)).tolist(), it.tolist()))
    assert got == sorted(map(tuple, quads.tolist()))
    got = sorted(zip(np.repeat(np.arange(n_ent), np.diff(op)).tolist(), ort[:, 0].tolist(), ort[:, 1].tolist(), ot.tolist()))
    assert got == sorted(map(tuple, quads.tolist()))
    # a valid call still works after the errors (marks empty: no edges)
    assert count(L.rg_texplain_count, fr_t, tg) == 0 and n_e.value == 0
    torch.cuda.synchronize()
