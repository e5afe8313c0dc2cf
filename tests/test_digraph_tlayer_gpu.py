"""rg_digraph_tlayer_fwd called on its own (-m gpu): one message-passing layer over an explicit, destination-segmented edge list with a
time per edge, in both of its forms - n_dir = 3, the interpolation layer (layer_ref.temporal_hop), and n_dir = 1, the extrapolation
form (layer_ref.windowed_hop, the test resolving each edge's day itself) - against the fp64 per-edge reference of tests/layer_ref.py,
under that file's error model unchanged:

    |agg - ref64| <= C_BOUND * (n + n0) * u * S + 1e-30                (layer_ref's docstring defines S, n, n0; C_BOUND = 1.6)

The edge lists are the CPU oracle's hops (layer_ref.hops; their time field from layer_ref.expand, which hops calls) re-ordered by
destination, so the reference sums every destination in the order the kernel is handed.  Every element is checked, pad columns
included; agg is pre-filled with NaN (every row must be written).
The kernel's worst ratio over these cases, as measured on an MI355X: 0.22 (the hub case; information only, the assertion uses C_BOUND).
Wall time of this file there: about 3 s (45 tests).
"""
import numpy as np
import pytest
import torch

from tests import layer_ref as lr

pytestmark = pytest.mark.gpu

KEYS = ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha")


def _dev(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x)).to(dtype).cuda()


def _arrays(e, etime, q_time, n_new):
    """The kernel's index arrays (numpy) of destination-ordered edges (batch, head, rel, tail, old_idx, new_idx) with their times."""
    ptr = np.zeros(n_new + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(e[:, 5], minlength=n_new))
    row_of = np.zeros(n_new, np.int64)
    row_of[e[:, 5]] = e[:, 0]
    return dict(dst_ptr=ptr.astype(np.int32), src_idx=e[:, 4].astype(np.int32), rel=e[:, 2].astype(np.int32),
                edge_time=np.asarray(etime).astype(np.int32), row_of_dst=row_of.astype(np.int32), q_time=np.asarray(q_time).astype(np.int32))


def _hops(case):
    """[(layer_ref hop, kernel arrays)] of the case's hops: layer_ref.hops' edge lists in destination order (stable: fact-row order
    inside one) with the time field layer_ref.expand returns next to them."""
    og, nodes, out = lr.oracle_graph(case), case.nodes0, []
    for old, new, edges, _ in lr.hops(case):
        new2, edges2, field = lr.expand(case, og, nodes)
        assert np.array_equal(edges2, edges) and np.array_equal(new2, new) and np.array_equal(nodes, old)
        order = np.argsort(edges[:, 5], kind="stable")
        e, field = np.asarray(edges, np.int64)[order], np.asarray(field, np.int64)[order]
        if case.kind == "temporal":
            hop = lr.temporal_hop(e, field, case.q_time, len(old), len(new), case.n_rela_rows, case.n_time)
            etime = field
        else:                                           # the field is the data row; the edge's day: the row's, a self-loop's: loop_time[b]
            hop = lr.windowed_hop(e, field, case.q_time, case.loop_time, case.row_time, case.n_data, case.n_tab, len(old), len(new))
            loop = field >= case.n_data
            etime = np.where(loop, case.loop_time[e[:, 0]], case.row_time[np.where(loop, 0, field)])
        out.append((hop, _arrays(e, etime, case.q_time, len(new))))
        nodes = new
    return out


def _n_dir(case):
    return 3 if case.kind == "temporal" else 1


def _call(case, A, X, ap=None, attn=None, want_alpha=True):
    """The raw entry point on numpy index arrays ``A`` and device inputs ``X``: (agg pre-filled with NaN, alpha or None)."""
    from red_gnn_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n_dst, E, n_dir = len(A["dst_ptr"]) - 1, len(A["src_idx"]), _n_dir(case)
    D = {k: _dev(v, torch.int32) for k, v in A.items()}
    agg = torch.full((n_dst, case.ld), float("nan"), dtype=torch.float32, device="cuda")
    alpha = torch.full((E,), float("nan"), dtype=torch.float32, device="cuda") if want_alpha else None
    nb = L.rg_digraph_layer_fwd_scratch_bytes(p(A["dst_ptr"]), n_dst, case.ld) if n_dst else 0
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
    assert X["hidden"].shape[0] == n_dir * X["a_s"].shape[0] and X["rela"].shape[0] == n_dir * X["a_r"].shape[0]
    _lib.check(L.rg_digraph_tlayer_fwd(n_dst, E, p(D["dst_ptr"]), p(A["dst_ptr"]), p(D["src_idx"]), p(D["rel"]), p(D["edge_time"]),
                                       p(D["row_of_dst"]), p(D["q_time"]), X["a_s"].shape[0], X["a_r"].shape[0], X["a_q"].shape[0],
                                       X["time_tab"].shape[0] // n_dir, n_dir, p(X["hidden"]), p(X["rela"]), p(X["time_tab"]), case.d, case.ld,
                                       p(X["a_s"]), p(X["a_r"]), p(X["a_q"]), case.ap if ap is None else ap, p(X["w_alpha"]), p(X["b_alpha"]),
                                       case.attn_dim if attn is None else attn, p(agg), p(alpha), p(scratch), nb, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return agg, alpha


def _check(tag, case, agg, f64):
    got = agg.cpu().numpy().astype(np.float64)
    assert not np.isnan(got).any(), "%s: %d elements of agg were never written" % (tag, int(np.isnan(got).sum()))
    n0 = lr.n0_of("agg", case.d, case.attn_dim)
    ok = np.abs(got - f64.agg) <= lr.bound(f64.S["agg"], f64.n["agg"], n0, lr.C_BOUND)
    ratio = lr.worst_ratio(got, f64.agg, f64.S["agg"], f64.n["agg"], n0)
    print("%s: worst ratio %.3g (allowed %.3g)" % (tag, ratio, lr.C_BOUND))
    assert ok.all(), "%s: %d of %d elements beyond the bound; worst ratio %.3g (allowed %.3g)" % (tag, int((~ok).sum()), ok.size, ratio,
                                                                                                lr.C_BOUND)
    assert not agg[:, case.d:].any(), tag + ": pad columns of agg"


def _run_hop(tag, case, k, hop, A):
    """One hop: the kernel against the reference, alpha against the reference's, two runs bit for bit, alpha_out = NULL."""
    x = lr.inputs(case, k, hop)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    f64 = lr.forward(hop, *(x[kk] for kk in KEYS))
    agg, alpha = _call(case, A, X)
    _check(tag, case, agg, f64)
    a = alpha.cpu().numpy().astype(np.float64)
    assert not np.isnan(a).any() and np.abs(a - f64.alpha).max() <= 1e-5, tag + ": alpha_out"
    again, alpha2 = _call(case, A, X)
    assert torch.equal(again, agg) and torch.equal(alpha2, alpha), tag + ": two runs differ"
    none, _ = _call(case, A, X, want_alpha=False)                         # alpha_out = NULL is accepted and changes nothing
    assert torch.equal(none, agg), tag
    return x, X, agg


def _run_case(case):
    for k, (hop, A) in enumerate(_hops(case)):
        out = _run_hop("%s hop %d" % (case.name, k + 1), case, k, hop, A)
    return (hop, A) + out


def _case(kind, name, d, ld, attn, ap=None, seed=0):
    make = lr._temporal_case if kind == "temporal" else lr._windowed_case
    c = make("%s_%s" % (kind, name), seed=seed, d=d, ld=ld, attn_dim=attn, B=5)
    if ap is not None:
        c.ap = ap
    return c


KINDS = ["temporal", "windowed"]                         # n_dir = 3, n_dir = 1


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d", [16, 20])
@pytest.mark.parametrize("ld", [32, 64, 128, 256])
def test_row_widths(kind, d, ld):
    _run_case(_case(kind, "d%d_ld%d" % (d, ld), d, ld, 5, seed=d + ld))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("attn,ap", [(3, 4), (5, 8), (16, 16), (17, 32), (3, 32), (5, 32), (16, 32)])
def test_attention_widths(kind, attn, ap):
    _run_case(_case(kind, "attn%d_ap%d" % (attn, ap), 16, 32, attn, ap=ap, seed=attn + ap))


@pytest.mark.parametrize("kind", KINDS)
def test_tight_rows_ld_equals_d(kind):
    _run_case(_case(kind, "d16_ld16", 16, 16, 5, seed=3))


def test_the_oracle_cases_hold_every_direction_and_both_clamps():
    """What the cases above are for: the temporal hops carry dt < 0, = 0, > 0 and |dt| = n_time - 1, the windowed ones a delta below 0
    and one past the table."""
    c = _case("temporal", "cover", 16, 32, 5, seed=1)
    dt = np.concatenate([hop.dt for hop, _ in _hops(c)])
    assert (dt < 0).any() and (dt == 0).any() and (dt > 0).any() and (np.abs(dt) == c.n_time - 1).any()
    c = _case("windowed", "cover", 16, 32, 5, seed=1)
    delta = np.concatenate([c.q_time[hop.b] - A["edge_time"] for hop, A in _hops(c)])
    assert (delta < 0).any() and (delta >= c.n_tab).any() and ((delta >= 0) & (delta < c.n_tab)).any()


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
def _hand_temporal(name, lengths, b_of, q_time, etime_of, seed, n_old=37, d=20, ld=32, attn=5):
    """A temporal hop typed in as destination lengths: destination o has lengths[o] edges, belongs to query b_of[o], its edges' times
    are etime_of(o, j); sources and relations are seeded random."""
    c = _case("temporal", name, d, ld, attn, seed=seed)
    rng = np.random.default_rng(seed)
    o = np.repeat(np.arange(len(lengths)), lengths)
    E = len(o)
    b = np.asarray(b_of)[o]
    s, r = rng.integers(0, n_old, E), rng.integers(0, c.n_rela_rows, E)
    etime = np.array([etime_of(int(oo), j) for oo, n in enumerate(lengths) for j in range(n)], np.int64)
    e = np.stack([b, np.zeros(E, np.int64), r, np.zeros(E, np.int64), s, o], 1)
    c.q_time = np.asarray(q_time, np.int64)
    assert len(c.q_time) == c.B
    hop = lr.temporal_hop(e, etime, c.q_time, n_old, len(lengths), c.n_rela_rows, c.n_time)
    return c, hop, _arrays(e, etime, c.q_time, len(lengths))


def test_one_destination_with_one_edge():
    c, hop, A = _hand_temporal("one_edge", [1], [1], [0, 7, 3, 3, 3], lambda o, j: 2, seed=5)
    x, X, agg = _run_hop("one edge", c, 0, hop, A)
    assert agg.shape == (1, c.ld) and hop.dir.tolist() == [0] and hop.trow.tolist() == [5]


@pytest.mark.parametrize("d,ld", [(20, 32), (64, 64), (20, 256)])           # 8, 16 and 64 lanes per destination
def test_cut_destinations_next_to_many_one_edge_destinations(d, ld):
    """Destinations of exactly 128 (the longest that is not cut), 129 and 257 edges (two and three chunks) among 600 one-edge
    destinations.  A destination's row does not depend on what else the call carries: the hubs alone, and each of them alone, give bit
    for bit the rows of the full call."""
    from red_gnn_amd import engine
    lengths = [1] * 200 + [128] + [1] * 200 + [129, 257] + [1] * 200
    c, hop, A = _hand_temporal("hubs", lengths, np.arange(len(lengths)) % 5, [0, 11, 5, 2, 8], lambda o, j: (7 * o + 5 * j) % 12, seed=6,
                               n_old=301, d=d, ld=ld)
    x, X, agg = _run_hop("hubs", c, 0, hop, A)
    assert engine.digraph_chunks(A["dst_ptr"]) == (2, 5, 257)
    length = np.diff(A["dst_ptr"].astype(np.int64))
    for pick in (np.nonzero(length > 1)[0], np.array([200]), np.array([401]), np.array([402]), np.arange(0, len(length), 3)):
        at = np.concatenate([np.arange(A["dst_ptr"][o], A["dst_ptr"][o + 1]) for o in pick])
        ptr = np.zeros(len(pick) + 1, np.int32)
        ptr[1:] = np.cumsum(length[pick])
        sub = dict(dst_ptr=ptr, src_idx=A["src_idx"][at], rel=A["rel"][at], edge_time=A["edge_time"][at], row_of_dst=A["row_of_dst"][pick],
                   q_time=A["q_time"])
        part, _ = _call(c, sub, X)
        assert torch.equal(part, agg[torch.as_tensor(pick).cuda()]), "a destination's row depends on the rest of the call"


def test_every_direction_and_the_longest_lag_on_hand_destinations():
    """Destination 0 (query time 5): edges at every time id, so dt < 0, = 0 and > 0; destination 1 (query time 0) and 2 (query time
    n_time - 1): |dt| = n_time - 1 in the future and in the past, next to dt = 0."""
    c, hop, A = _hand_temporal("directions", [12, 2, 2], [2, 0, 1], [0, 11, 5, 3, 3], lambda o, j: j if o == 0 else 11 * j, seed=7)
    first = hop.o == 0
    assert set(hop.dir[first].tolist()) == {0, 1, 2} and hop.dt[~first].tolist() == [0, 11, -11, 0]
    assert hop.trow[~first].tolist() == [c.n_time, 2 * c.n_time + 11, 11, c.n_time]
    _run_hop("directions", c, 0, hop, A)


def test_times_outside_the_table_are_clamped_into_it():
    """The raw entry point (the wrapper refuses such times): an edge time far outside 0..n_time-1 reads the direction's last row."""
    c, hop, A = _hand_temporal("clamped", [4], [0], [3, 3, 3, 3, 3], lambda o, j: (3, 14, 10 ** 9, -2 ** 31)[j], seed=8)
    assert hop.dt.tolist() == [0, 11, 10 ** 9 - 3, -2 ** 31 - 3]
    hop.trow = hop.dir * c.n_time + np.minimum(np.abs(hop.dt), c.n_time - 1)
    assert hop.trow.tolist() == [12, 35, 35, 11]
    _run_hop("clamped", c, 0, hop, A)


def test_extrapolation_form_clamps_the_lag_at_both_ends():
    """n_dir = 1: query day 10, a table of 6 lags; edges on days 15 (delta -5: row 0), 10 (row 0), 6 (row 4), 5 (row 5, the last), 4 and 0
    (deltas 6 and 10: row 5)."""
    c = _case("windowed", "lags", 20, 32, 5, seed=9)
    days = np.array([15, 10, 6, 5, 4, 0, 9, 30])
    lengths, b_of = [6, 2], [1, 4]
    c.q_time = np.array([3, 10, 3, 3, 8])
    o = np.repeat(np.arange(2), lengths)
    E, n_old = len(o), 9
    rng = np.random.default_rng(9)
    e = np.stack([np.asarray(b_of)[o], np.zeros(E, np.int64), rng.integers(0, c.n_rela_rows, E), np.zeros(E, np.int64),
                  rng.integers(0, n_old, E), o], 1)
    hop = lr.windowed_hop(e, np.arange(E), c.q_time, np.zeros(c.B, np.int64), days, E, c.n_tab, n_old, 2)      # data rows 0..E-1, no loops
    assert c.n_tab == 6 and hop.trow.tolist() == [0, 0, 4, 5, 5, 5, 0, 0]
    _run_hop("lags", c, 0, hop, _arrays(e, days, c.q_time, 2))


def test_no_edges_launches_nothing():
    from red_gnn_amd import _lib
    c, hop, A = _hand_temporal("none", [1], [1], [0, 7, 3, 3, 3], lambda o, j: 2, seed=5)
    X = {kk: _dev(v) for kk, v in lr.inputs(c, 0, hop).items() if v is not None}
    empty = dict(dst_ptr=np.zeros(4, np.int32), src_idx=np.zeros(0, np.int32), rel=np.zeros(0, np.int32), edge_time=np.zeros(0, np.int32),
                 row_of_dst=np.zeros(3, np.int32), q_time=A["q_time"])
    agg, alpha = _call(c, empty, X)
    assert torch.isnan(agg).all() and alpha.numel() == 0          # success, and agg_out is left alone
    assert _lib.lib().rg_digraph_tlayer_fwd(*([0, 0] + [None] * 7 + [0, 0, 0, 12, 3, None, None, None, 16, 16, None, None, None, 4, None, None,
                                                                   3] + [None] * 3 + [0, None])) == 0


def test_unsupported_attention_width_is_an_error_and_the_next_call_is_fine():
    from red_gnn_amd import _lib
    c, hop, A = _hand_temporal("ap20", [3, 130, 1], [0, 1, 2], [0, 11, 5, 3, 3], lambda o, j: (o + j) % 12, seed=10)
    x = lr.inputs(c, 0, hop)
    good = {kk: _dev(v) for kk, v in x.items() if v is not None}
    c.attn_dim = c.ap = 20
    X = {kk: _dev(v) for kk, v in lr.inputs(c, 0, hop).items() if v is not None}
    with pytest.raises(_lib.NativeError, match="padded attention dim 20"):
        _call(c, A, X)
    c.attn_dim, c.ap = 5, 8
    agg, _ = _call(c, A, good)
    _check("after the error", c, agg, lr.forward(hop, *(x[kk] for kk in KEYS)))


@pytest.mark.parametrize("kind", KINDS)
def test_engine_wrapper_checks_and_matches(kind):
    """engine.digraph_tlayer_fwd: the raw call's bits, zero rows for destinations without edges, E == 0, DIGRAPH_EVENTS, and ValueError
    for indices and times outside their ranges."""
    from red_gnn_amd import engine
    case = _case(kind, "wrapper", 20, 32, 5, seed=6)
    hop, A = _hops(case)[1]
    n_dir = _n_dir(case)
    x = lr.inputs(case, 1, hop)
    X = {kk: _dev(v) for kk, v in x.items() if v is not None}
    raw, raw_alpha = _call(case, A, X)
    D = {k: _dev(v, torch.int32) for k, v in A.items()}
    tabs = (X["hidden"], X["rela"], X["time_tab"], case.d, X["a_s"], X["a_r"], X["a_q"], X["w_alpha"], X["b_alpha"], case.attn_dim)
    run = lambda a, **kw: engine.digraph_tlayer_fwd(a["dst_ptr"], a["src_idx"], a["rel"], a["row_of_dst"], *tabs, edge_time=a["edge_time"],
                                                    q_time=a["q_time"], **{"n_dir": n_dir, **kw})
    engine.DIGRAPH_EVENTS = []
    try:
        agg, alpha = run(D)
        events = engine.DIGRAPH_EVENTS
    finally:
        engine.DIGRAPH_EVENTS = None
    assert torch.equal(agg, raw) and torch.equal(alpha, raw_alpha)
    assert len(events) == 1 and events[0][2:] == (len(A["dst_ptr"]) - 1, len(A["src_idx"]))
    torch.cuda.synchronize()
    assert events[0][0].elapsed_time(events[0][1]) >= 0.0
    agg_na, none = run(D, want_alpha=False)
    assert none is None and torch.equal(agg_na, raw)
    # two destinations without edges appended: their rows are zero, the others keep their bits
    more = dict(D, dst_ptr=torch.cat([D["dst_ptr"], D["dst_ptr"][-1:].repeat(2)]),
                row_of_dst=torch.cat([D["row_of_dst"], torch.zeros(2, dtype=torch.int32, device="cuda")]))
    agg2, _ = run(more)
    assert torch.equal(agg2[:-2], raw) and not agg2[-2:].any()
    none = torch.zeros(0, dtype=torch.int32, device="cuda")
    agg0, alpha0 = run(dict(D, dst_ptr=torch.zeros(4, dtype=torch.int32, device="cuda"), src_idx=none, rel=none, edge_time=none,
                            row_of_dst=more["row_of_dst"][:3]))
    assert agg0.shape == (3, case.ld) and not agg0.any() and alpha0.numel() == 0
    bad_time = X["time_tab"].shape[0] // 3 if n_dir == 3 else -1              # n_dir 3: a time id; n_dir 1: any day from 0 on
    for name, bad in (("src_idx", X["a_s"].shape[0]), ("rel", X["a_r"].shape[0]), ("row_of_dst", X["a_q"].shape[0]), ("src_idx", -1),
                      ("edge_time", bad_time), ("edge_time", -1)):
        args = dict(D)
        args[name] = D[name].clone()
        args[name][0] = bad
        with pytest.raises(ValueError, match=name + " out of range"):
            run(args)
    if n_dir == 1:                                                            # a day beyond the table is in order: the lag is clamped
        far = dict(D, edge_time=D["edge_time"] + 1000)
        assert run(far)[0].shape == raw.shape
    for n in (2, 0, True, 3.0):
        with pytest.raises(ValueError, match="n_dir must be 1 or 3"):
            run(D, n_dir=n)
    with pytest.raises(ValueError, match="do not fit together"):
        run(D, n_dir=4 - n_dir)                                               # the other form's table shapes
    with pytest.raises(ValueError, match="edge_time must be an int32 vector"):
        run(dict(D, edge_time=D["edge_time"].long()))
    with pytest.raises(ValueError, match="do not fit together"):
        run(dict(D, q_time=D["q_time"][:-1].contiguous()))
    with pytest.raises(ValueError, match="contiguous and on the device"):
        run(dict(D, edge_time=D["edge_time"].cpu()))
