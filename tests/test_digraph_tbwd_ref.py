"""tests/digraph_tbwd_ref.py on its own (no GPU): the fp32 run of the reference stays within layer_ref.REF32_WORST_RATIO of the fp64 run
under layer_ref's error model on every hop the timed kernel's tests use, grad_gate's model included; the gate gradient is the
derivative it claims to be (agg is linear in the gates); the grouped attention rows are layer_ref's grad_a_s; and the hops, the
directed view and the hand-built lists are what the kernel's tests assume."""
import types

import numpy as np

from tests import digraph_tbwd_ref as T
from tests import layer_ref as lr

_HOPS = {}


def _hops():
    if not _HOPS:
        _HOPS.update({tag: (c, k, hop, A) for tag, c, k, hop, A in T.all_hops()})
    return _HOPS


def test_fp32_reference_within_its_bound_on_every_case():
    worst = dict.fromkeys(T.OUTPUTS, 0.0)
    for tag, (c, k, hop, A) in _hops().items():
        x = T.inputs(c, k, hop)
        r64, r32 = T.backward(hop, *T.tables(x)), T.backward(hop, *T.tables(x), dtype=np.float32)
        here = {}
        for name in T.OUTPUTS:
            assert getattr(r32, name).dtype == np.float32
            ratio = lr.worst_ratio(getattr(r32, name), getattr(r64, name), r64.S[name], r64.n[name], T.n0_of(name, c.d, c.attn_dim))
            worst[name], here[name] = max(worst[name], ratio), ratio
            assert ratio <= lr.REF32_WORST_RATIO, "%s %s: fp32 reference at ratio %.3g" % (tag, name, ratio)
        print("%s: E %d, ratios %s" % (tag, hop.E, {n: "%.3g" % v for n, v in here.items()}))
    print("worst ratios of the fp32 reference: %s (allowed %.3g)" % (worst, lr.REF32_WORST_RATIO))


def _without(hop, e):
    """The hop without edge e."""
    keep = np.arange(hop.E) != e
    cut = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape == (hop.E,) else v) for k, v in hop.__dict__.items() if k != "oracle"}
    return types.SimpleNamespace(**{**cut, "E": hop.E - 1})


def test_gate_gradient_is_what_the_edge_adds_to_the_sums():
    """agg is linear in the gates, so <G, agg> with edge e dropped (g_e = 0) differs from the full sum by grad_gate[e]: both timed
    forms, the clamped hops included, in fp64 to 1e-12."""
    for tag in ("n_dir3_d20_ld32 hop 2", "n_dir1_d20_ld32 hop 2", "clamped_n_dir3", "clamped_n_dir1"):
        c, k, hop, A = _hops()[tag]
        x = T.inputs(c, k, hop)
        fwd = lambda h: lr.forward(h, x["hidden"], x["rela"], x["time_tab"], x["a_s"], x["a_r"], x["a_q"], x["w_alpha"], x["b_alpha"]).agg
        G = x["grad_agg"].astype(np.float64)
        full, want = fwd(hop), T.backward(hop, *T.tables(x)).grad_gate
        picks = np.unique(np.concatenate([np.random.default_rng(0).integers(0, hop.E, 12), [0, 1, 2, hop.E - 1]]))
        for e in picks:
            o = hop.o[e]
            diff = float((G[o] * (full[o] - fwd(_without(hop, e))[o])).sum())
            assert abs(diff - want[e]) <= 1e-12 * max(1.0, abs(want[e])), "%s edge %d: %.17g against %.17g" % (tag, e, diff, want[e])


def test_grouped_attention_rows_are_layer_refs_grad_a_s():
    """The kernel's rows per directed source, added per source, are layer_ref.backward's grad_a_s on the hop as it stands; grad_hidden
    is layer_ref's as it is."""
    for tag in ("n_dir3_d20_ld32 hop 2", "n_dir1_d20_ld32 hop 2", "hub_rows_n_dir3", "clamped_n_dir3"):
        c, k, hop, A = _hops()[tag]
        x = T.inputs(c, k, hop)
        mine = T.backward(hop, *T.tables(x))
        theirs = lr.backward(hop, *T.tables(x))
        assert mine.grad_a_s_dir.shape == (hop.n_dir * hop.n_old, c.ap)
        np.testing.assert_allclose(T.group_directions(mine.grad_a_s_dir, hop.n_dir), theirs.grad_a_s, rtol=1e-12, atol=1e-14)
        assert np.array_equal(mine.grad_hidden, theirs.grad_hidden)
        if hop.n_dir == 1:
            assert np.array_equal(mine.grad_a_s_dir, theirs.grad_a_s)


def test_hops_from_the_kernels_arrays_are_layer_refs():
    """timed_hop on the arrays the kernel takes forms the rows layer_ref's temporal_hop / windowed_hop form on the oracle's edges."""
    seen = set()
    for tag, (c, k, hop, A) in _hops().items():
        if not hasattr(hop, "oracle"):
            continue
        for name in ("b", "s", "r", "o", "hrow", "rrow", "trow"):
            assert np.array_equal(getattr(hop, name), getattr(hop.oracle, name)), "%s: %s" % (tag, name)
        assert hop.n_old == hop.oracle.n_old and hop.n_new == hop.oracle.n_new and (np.diff(hop.o) >= 0).all()
        if hop.n_dir == 3:
            seen |= set(hop.dir.tolist())
        else:                       # the windowed case clamps on both sides by itself
            lag = np.asarray(c.q_time, np.int64)[hop.b] - A["edge_time"]
            seen |= {"neg"} if (lag < 0).any() else set()
            seen |= {"long"} if (lag >= c.n_tab_rows).any() else set()
    assert seen >= {0, 1, 2, "neg", "long"}


def test_directed_view_and_the_hand_built_hops():
    for n_dir in T.N_DIRS:
        c, hop, A = T.hub_hop(n_dir)
        V = T.directed_view(hop)
        deg = np.diff(V["src_ptr"].astype(np.int64))
        assert deg[:9].tolist() == list(T.HUB_DEGREES) + [0] and (deg[9:9 + 1000] == 1).all() and len(deg) == n_dir * hop.n_old
        assert np.array_equal(np.sort(V["edge_of"]), np.arange(hop.E))
        for u in range(9):
            mine = V["edge_of"][V["src_ptr"][u]:V["src_ptr"][u + 1]]
            assert (hop.hrow[mine] == u).all() and (np.diff(mine) > 0).all()          # the row's edges, in list order
        assert (np.diff(hop.o) >= 0).all() and A["edge_time"].min() >= 0
        if n_dir == 3:                                                                # two of three directions: sources 0 and 2
            assert A["edge_time"].max() < c.n_tab_rows
            assert set(hop.dir[hop.s == 0].tolist()) == {1, 2} and set(hop.dir[hop.s == 2].tolist()) == {0, 1}
        A2, at = T.take_rows(A, hop, np.arange(0, len(deg), 3))
        hop2 = T.timed_hop(A2, c.q_time, n_dir, hop.n_old, c.n_rela_rows, c.n_tab_rows)
        assert np.array_equal(hop2.hrow, hop.hrow[at]) and np.array_equal(hop2.o, hop.o[at]) and np.array_equal(hop2.trow, hop.trow[at])
    # the clamped hops: times outside the table, rows inside it
    c, k, hop, A, at = T.clamped_hop(3)
    dt = A["edge_time"][at].astype(np.int64) - np.asarray(c.q_time)[hop.b[at]]
    assert (np.abs(dt) >= c.n_tab_rows).all() and (dt > 0).any() and (dt < 0).any()
    assert (hop.trow[at] == hop.dir[at] * c.n_tab_rows + c.n_tab_rows - 1).all() and hop.trow.max() < 3 * c.n_tab_rows
    c, k, hop, A, at = T.clamped_hop(1)
    lag = np.asarray(c.q_time)[hop.b[at]] - A["edge_time"][at].astype(np.int64)
    assert lag[0] < 0 and lag[1] >= c.n_tab_rows and hop.trow[at].tolist() == [0, c.n_tab_rows - 1]
    c, hop, A = T.one_edge_hop(3)
    assert hop.hrow.tolist() == [11] and hop.trow.tolist() == [2 * 12 + 2]
    c, hop, A = T.one_edge_hop(1)
    assert hop.hrow.tolist() == [3] and hop.trow.tolist() == [0]


def test_reference_on_a_typed_in_hop():
    """Two edges into one destination from one source, d = 1, no attention input: alpha = 1/2.  The first edge lies in the past of
    the query (dt = -1), the second in its future (dt = +2)."""
    A = dict(dst_ptr=np.array([0, 2], np.int32), src_idx=np.array([0, 0], np.int32), rel=np.array([0, 1], np.int32),
             row_of_dst=np.array([0], np.int32), edge_time=np.array([2, 5], np.int32))
    hop = T.timed_hop(A, np.array([3]), 3, 1, 2, 4)
    assert hop.hrow.tolist() == [0, 2] and hop.rrow.tolist() == [0, 2 * 2 + 1] and hop.trow.tolist() == [1, 2 * 4 + 2]
    hidden = np.array([[2.0], [100.0], [-1.0]])
    rela = np.arange(6, dtype=np.float64).reshape(6, 1)          # rows 0 and 5: 0 and 5
    time_tab = np.arange(12, dtype=np.float64).reshape(12, 1) * 10      # rows 1 and 10: 10 and 100
    zero = np.zeros((1, 4))
    r = T.backward(hop, hidden, rela, time_tab, zero, np.zeros((2, 4)), zero, np.array([1.0]), np.array([0.0]), np.array([[4.0]]))
    assert np.allclose(r.grad_gate, [0.5 * 4 * (2 + 0 + 10), 0.5 * 4 * (-1 + 5 + 100)])
    assert np.allclose(r.grad_hidden, [[0.5 * 4], [0.0], [0.5 * 4]]) and not r.grad_a_s_dir.any()          # relu'(0) = 0
    assert np.allclose(r.S["grad_gate"], [0.5 * 4 * 12, 0.5 * 4 * 106]) and r.n["grad_gate"].tolist() == [1, 1]
    V = T.directed_view(hop)
    assert V["src_ptr"].tolist() == [0, 1, 1, 2] and V["edge_of"].tolist() == [0, 1]
