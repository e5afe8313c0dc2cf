"""tests/hop_ref.py checked on the CPU: the dense hop reference against python loops on a hand-made graph and against the oracle's hop
lists on every case, the conditions the GPU tests rely on (the profile's words per wave step, the LDS budget of the extrapolation
profile, the share of singleton edges of the one-hot readout) and the alpha bound against a plain fp32 evaluation."""
import functools
import types

import numpy as np
import pytest

from tests import hop_ref as hr
from tests import layer_ref as lr


@functools.lru_cache(maxsize=None)
def _case_hops(name):
    case = hr.CASES[name]()
    return case, lr.oracle_graph(case), lr.hops(case)


def _rows_sorted(*cols):
    a = np.stack([np.asarray(c, np.int64) for c in cols], 1)
    return a[np.lexsort(a.T[::-1])]


def _hand_graph():
    """40 entities (two bitmap words: entities 31, 32 and 39 sit at the words' edges), 9 data rows + one self-loop per entity."""
    data = [(1, 0, 2), (1, 0, 2),        # rows 0, 1: a repeated fact
            (3, 1, 2),                   # row 2
            (31, 2, 32),                 # row 3
            (32, 3, 39),                 # row 4
            (3, 1, 39),                  # row 5
            (1, 2, 39),                  # row 6
            (0, 0, 31),                  # row 7
            (7, 1, 6)]                   # row 8: its head is in no level
    n_ent, n_data = 40, len(data)
    quads = [(h, r, t, i) for i, (h, r, t) in enumerate(data)] + [(e, 4, e, n_data) for e in range(n_ent)]
    return n_ent, n_data, lr.quad_graph(quads, n_ent, 5)


def test_hop_reference_against_loops_by_hand():
    n_ent, n_data, og = _hand_graph()
    in_ptr, in_hr, in_time = hr.csr_by_tail(og)
    B = 2
    level_old = {(0, e) for e in (0, 1, 3, 31, 32)} | {(1, e) for e in (1, 32, 39)}
    # tail 6: in-edges, none from the level before; tail 9: its self-loop only, and 9 is not in the level before
    marked = {(0, e) for e in (2, 6, 9, 31, 32, 39)} | {(1, e) for e in (0, 2, 39)}
    # row 0's window [2, 5): row 2 sits at win_lo, row 4 at win_hi - 1, row 5 at win_hi; row 1 sees every row
    win_lo, win_hi = np.array([2, 0]), np.array([5, n_data])
    alpha_of = lambda b, h, r: np.float32(((7 * b + 3 * h + 5 * r) % 16) / 16.0)
    nodes_old = np.array(sorted(level_old))
    marks = hr.bitmap(sorted(marked), B, n_ent)
    assert marks[0].tolist() == [(1 << 2) | (1 << 6) | (1 << 9) | (1 << 31), (1 << 0) | (1 << 7)]
    assert np.array_equal(hr.bitmap_nodes(marks), np.array(sorted(marked)))
    for kind in ("windowed", "static"):
        case = types.SimpleNamespace(kind=kind, B=B, n_ent=n_ent, n_data=n_data, win_lo=win_lo, win_hi=win_hi)
        gx = (in_ptr, in_hr, in_time if kind == "windowed" else None)
        window = (win_lo, win_hi, n_data) if kind == "windowed" else None
        every = hr.expected_hop_edges(case, gx, nodes_old, marks)
        tab = hr.AlphaTable(n_ent, 5, every.edges[:, 0], every.edges[:, 1], every.edges[:, 2],
                            np.array([alpha_of(*e[:3]) for e in every.edges], np.float32))
        a = alpha_of(0, 3, 1)                  # 0.875: the alpha of (0, 3, 1, 2), an edge of both kinds
        for tau in (-np.inf, 0.0, np.float32(0.5), a, np.nextafter(a, np.float32(np.inf)), np.inf):
            want, heads = hr.brute_hop_edges(B, n_ent, in_ptr, in_hr, in_time, level_old, marked, alpha_of, tau, window)
            got = hr.expected_hop_edges(case, gx, nodes_old, marks, tab, tau)
            assert [tuple(e) + (p,) for e, p in zip(got.edges.tolist(), got.pos.tolist())] == want, (kind, tau)
            assert np.array_equal(got.heads, hr.bitmap(sorted(heads), B, n_ent)), (kind, tau)
            assert got.word_count.sum() == len(want)
            assert np.array_equal(nodes_old[got.old_idx], got.edges[:, :2])
        rows = [tuple(e) for e in every.edges.tolist()]
        assert (0, 6) not in {(b, t) for b, _, _, t in rows} and (0, 9) not in {(b, t) for b, _, _, t in rows}
        assert rows.count((1, 1, 0, 2)) == 2                                       # the repeated fact, once per row
        assert {(0, 31, 4, 31), (0, 32, 4, 32), (1, 39, 4, 39)} <= set(rows)       # self-loops pass every window
        in_window = [(0, 3, 1, 2) in rows, (0, 32, 3, 39) in rows, (0, 3, 1, 39) in rows, (0, 1, 0, 2) in rows]
        assert in_window == ([True, True, False, False] if kind == "windowed" else [True, True, True, True])
        # tau equal to an alpha keeps its edges, the next float drops them and nothing else
        hit = [e for e in every.edges.tolist() if alpha_of(*e[:3]) == a]
        assert hit
        keep = hr.expected_hop_edges(case, gx, nodes_old, marks, tab, a).edges.tolist()
        drop = hr.expected_hop_edges(case, gx, nodes_old, marks, tab, np.nextafter(a, np.float32(np.inf))).edges.tolist()
        assert all(e in keep for e in hit) and not any(e in drop for e in hit) and len(keep) - len(drop) == len(hit)


def test_profile_reference_by_hand():
    """Half to even at 2^-33, the three layouts and the dropped lag bin."""
    a = np.array([0.5, 2.0 ** -33, 3 * 2.0 ** -33, 1.0, 0.0, 0.75], np.float32)
    assert hr.fixed_point(a).tolist() == [1 << 31, 0, 2, 1 << 32, 0, 3 << 30]
    hop = types.SimpleNamespace(b=np.array([0, 0, 1, 1, 1, 0]), r=np.array([2, 2, 0, 2, 2, 1]), dir=np.array([0, 2, 1, 1, 1, 0]),
                                trow=np.array([0, 1, 2, 3, 3, 1]))
    s, c = hr.expected_profile(hop, a, 2, 3)
    assert c.tolist() == [[0, 1, 2], [1, 0, 2]] and s.tolist() == [[0, 3 << 30, 1 << 31], [2, 0, 1 << 32]]
    s, c = hr.expected_profile(hop, a, 2, 3, "temporal")
    assert c.shape == (2, 3, 3) and c[0, 0].tolist() == [0, 1, 1] and c[0, 2, 2] == 1 and c[1, 1].tolist() == [1, 0, 2] and c.sum() == 6
    assert s[0, 0, 2] == 1 << 31 and s[0, 2, 2] == 0 and s[1, 1, 2] == 1 << 32
    s, c = hr.expected_profile(hop, a, 2, 3, "windowed", lag_bin=np.array([0, 1, 1, 9]), n_bins=2)
    assert c.sum() == 4 and c[1].sum() == 1 and c[1, 1, 0] == 1 and c[0, 1].tolist() == [0, 1, 1] and s[0, 0, 2] == 1 << 31


def test_singleton_mask_by_hand():
    hop = types.SimpleNamespace(o=np.array([0, 0, 0, 1, 1]), r=np.array([1, 5, 2, 1, 1]))
    assert hr.singleton_mask(hop, 4).tolist() == [False, False, True, False, False]      # 1 and 5 share a column at d = 4
    assert hr.singleton_mask(hop, 8).tolist() == [True, True, True, False, False]


def test_words_per_wave_step():
    assert [hr.gw_of(1024, n) for n in hr.GW_CASES.values()] == [8, 16, 32, 64]
    assert [hr.n_words(n) for n in hr.GW_CASES.values()] == [65, 129, 257, 513]
    assert [int(name[2:]) for name in hr.GW_CASES] == [8, 16, 32, 64]
    assert hr.gw_of(64, 10000) == 4                   # the largest profile shape of the model-level tests
    others = {name: hr.gw_of(hr.CASES[name]().B, hr.CASES[name]().n_ent) for name in ("default", "hubs", "tickets")}
    assert set(others.values()) == {4}, others
    assert hr.gw_of(3, (1 << 20) + 37) == 8           # the wide-entity cases: 3 * ceil(32770 / 8) = 12291 pieces


@pytest.mark.parametrize("name", list(hr.GW_CASES))
def test_gw_cases_iterate_both_loops(name):
    case, og, hops = _case_hops(name)
    assert (case.B, case.hops, hr.gw_of(case.B, case.n_ent)) == (1024, 1, int(name[2:]))
    old, new, edges, hop = hops[0]
    heads, out_edges = hr.dense_steps(case, old, np.diff(og.head_ptr))
    print("%s: E %d, most heads in a wave step %d, most out-edges of 64 of them %d" % (name, hop.E, heads, out_edges))
    assert heads > 64 and out_edges > 64
    assert heads <= 32 * hr.gw_of(case.B, case.n_ent)
    assert 2000 <= hop.E <= 60000


def test_extrapolation_lds_budget():
    case = hr.CASES[hr.XLDS]()
    assert (case.kind, case.n_rela_rows, case.ap, case.n_tab) == ("windowed", 463, 8, hr.XLDS_BINS)
    assert 65536 < hr.xlds_bytes(case.n_rela_rows, case.ap, hr.XLDS_BINS, case.n_tab) <= 81920
    assert 65536 < 16384 + 463 * (4 * 8 + 12 * 8) + 8 == 75656 <= 81920
    w = hr.CASES["windowed"]()
    assert hr.xlds_bytes(w.n_rela_rows, w.ap, w.n_tab, w.n_tab) < 65536      # the small windowed case: the default launch


@pytest.mark.parametrize("name", list(hr.CASES))
def test_reference_on_every_case(name):
    """Per hop: all of level l marked and tau = 0 give the oracle's hop as a multiset (old index and time field included) and every
    level-(l-1) node as a head; at least half of the edges are singletons of the one-hot readout, and the fp64 forward with the one-hot
    tables holds exactly their alpha at agg[o, r % d]; a plain fp32 alpha stays within the bound the GPU tests use."""
    case, og, hops = _case_hops(name)
    gx = hr.csr_by_tail(og)
    for k, (old, new, edges, hop) in enumerate(hops):
        tag = "%s hop %d" % (name, k + 1)
        exp = hr.expected_hop_edges(case, gx, old, hr.bitmap(new, case.B, case.n_ent))
        assert len(exp.edges) == hop.E, tag
        if case.kind == "static":
            assert np.array_equal(_rows_sorted(*exp.edges.T, exp.old_idx), _rows_sorted(*edges[:, :5].T)), tag
        else:
            # the oracle's time field: re-read from the graph's rows through the edge's (head, rel, tail) is ambiguous for repeated
            # facts, so the hop objects are compared instead: dir / trow are functions of the time field
            exp_hop = lr.hop_of(case, np.column_stack([exp.edges, exp.old_idx, np.zeros(len(exp.edges), np.int64)]), exp.time, len(old), len(new))
            extra = (exp_hop.dir, hop.dir) if case.kind == "temporal" else (exp_hop.trow, hop.trow)
            assert np.array_equal(_rows_sorted(*exp.edges.T, exp.old_idx, extra[0], exp_hop.trow), _rows_sorted(*edges[:, :5].T, extra[1], hop.trow)), tag
        assert np.array_equal(exp.heads, hr.bitmap(old, case.B, case.n_ent)), tag
        assert np.array_equal(bitmap_of_tails(exp, case), hr.bitmap(new, case.B, case.n_ent)), tag

        single = hr.singleton_mask(hop, case.d)
        share = single.mean()
        x = lr.inputs(case, k, hop)
        a64, kap, bnd = hr.alpha_ref(case, hop, x)
        y = hr.one_hot_tables(case, x)
        agg = lr.forward(hop, *(y[kk] for kk in hr.KEYS)).agg
        assert np.array_equal(agg[hop.o[single], hop.r[single] % case.d], a64[single]), tag
        a32 = lr.forward(hop, *(x[kk] for kk in hr.KEYS), dtype=np.float32).alpha
        assert a32.dtype == np.float32
        ratio = hr.alpha_ratio(a32, a64, kap, case)
        print("%s (E %d): singleton share %.3f, fp32 alpha worst ratio %.3g (allowed %.3g)" % (tag, hop.E, share, ratio, lr.C_BOUND))
        assert share >= 0.5, tag
        assert (np.abs(a32.astype(np.float64) - a64) <= bnd).all(), (tag, ratio)


def bitmap_of_tails(exp, case):
    return hr.bitmap(exp.edges[:, [0, 3]], case.B, case.n_ent)
