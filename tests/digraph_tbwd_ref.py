"""Per-edge reference of rg_digraph_tlayer_bwd - the adjoint of ONE rg_digraph_tlayer_fwd hop, in both timed forms (n_dir = 3, temporal
interpolation; n_dir = 1, the extrapolation form), with respect to a gate on every edge's message, the directed source states and the
sources' attention projection - in plain numpy, fp64 and fp32, and the cases the kernel's tests share.  TEST INFRASTRUCTURE.

Everything sits on tests/layer_ref.backward, which knows both timed forms (temporal_hop / windowed_hop): grad_hidden is its grad_hidden
(by directed row hrow), and grad_a_s_dir - the kernel's attention rows, one per DIRECTED source row - is its grad_a_s on the same hop
with the source renamed to the directed row (s := hrow, a_s repeated n_dir times), so S, n and n0 are layer_ref's, unchanged.  Summed
over a source's directions it is layer_ref's grad_a_s on the hop as it stands (test_digraph_tbwd_ref.py).  grad_gate is added under the
rule of tests/digraph_bwd_ref.py, the message now holding the time row: per edge e = (b, s, r, o), G = grad_agg,

    m_e          = hidden[hrow] + rela[rrow] + time_tab[trow]
    grad_gate[e] = alpha_e * <G[o], m_e>
    S            = kappa_e * sum_j |G[o]_j| (|hidden[hrow]_j| + |rela[rrow]_j| + |time_tab[trow]_j|)
    n            = 1
    n0           = attn_dim + 6 + d                                              as digraph_bwd_ref has it

The third term of the message is one more add per column; it did not need a larger n0: measured over every case below
(test_digraph_tbwd_ref.py prints the per-case figures) the fp32 run of this file stays within |ref32 - ref64| / ((n + n0) u S) <= 0.06
for grad_gate, 0.18 for grad_hidden and 0.014 for grad_a_s_dir, under layer_ref.REF32_WORST_RATIO = 0.4.  C_BOUND is layer_ref's.

A hop is described by the arrays the kernel takes (``A``: dst_ptr, src_idx, rel, row_of_dst, edge_time in destination order, plus
q_time); timed_hop forms hrow / rrow / trow from them exactly as the kernel does - 64-bit differences, |dt| clamped to n_time - 1, the
n_dir = 1 lag clamped to 0 .. n_time - 1 - so that it also describes times outside the table.
"""
import types

import numpy as np

from tests import digraph_bwd_ref as D
from tests import layer_ref as lr

OUTPUTS = ("grad_gate", "grad_hidden", "grad_a_s_dir")


def n0_of(name, d, attn_dim):
    return D.n0_of("grad_a_s" if name == "grad_a_s_dir" else name, d, attn_dim)


# ---- a hop from the kernel's arrays ----------------------------------------------------------------------------------------------------
def dst_of_edge(A):
    return np.repeat(np.arange(len(A["dst_ptr"]) - 1), np.diff(A["dst_ptr"].astype(np.int64)))


def timed_hop(A, q_time, n_dir, n_old, n_rela_rows, n_time):
    """The layer_ref hop of the kernel's arrays, rows clamped as the kernel clamps them."""
    o = dst_of_edge(A)
    b = A["row_of_dst"].astype(np.int64)[o]
    s, r = A["src_idx"].astype(np.int64), A["rel"].astype(np.int64)
    et, qt = A["edge_time"].astype(np.int64), np.asarray(q_time, np.int64)[b]
    if n_dir == 3:
        dt = et - qt
        dirn = np.where(dt > 0, 2, np.where(dt == 0, 1, 0))
        hrow, rrow, trow = 3 * s + dirn, dirn * n_rela_rows + r, dirn * n_time + np.minimum(np.abs(dt), n_time - 1)
    else:
        dirn = np.zeros(len(s), np.int64)
        hrow, rrow, trow = s, r, np.clip(qt - et, 0, n_time - 1)
    return types.SimpleNamespace(kind="temporal" if n_dir == 3 else "windowed", b=b, s=s, r=r, o=o, hrow=hrow, rrow=rrow, trow=trow,
                                 n_old=int(n_old), n_new=len(A["dst_ptr"]) - 1, E=len(s), dir=dirn, n_dir=n_dir)


def directed_view(hop):
    """The source view segmented by the DIRECTED source row (hop.hrow): src_ptr [n_dir * n_old + 1], edge_of [E] (the stable sort by
    directed row) and dst_of_edge [E], int32."""
    n_rows = hop.n_dir * hop.n_old
    ptr = np.zeros(n_rows + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(hop.hrow, minlength=n_rows))
    return dict(src_ptr=ptr.astype(np.int32), edge_of=np.argsort(hop.hrow, kind="stable").astype(np.int32), dst_of_edge=hop.o.astype(np.int32))


def _gate(hop, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, G_rows, absolute):
    _, _, alpha = lr._attention(hop, a_s, a_r, a_q, w_alpha, b_alpha)
    G = G_rows[hop.o]
    if absolute:
        G, alpha = np.abs(G), lr._kappa(hop, a_s, a_r, a_q, w_alpha, b_alpha, alpha)
    return alpha * (G * lr._message(hop, hidden, rela, time_tab, absolute)).sum(1, dtype=G.dtype)


def directed_sources(hop):
    """The same hop with every directed row a source of its own (s := hrow): layer_ref.backward then sums grad_a_s per directed row."""
    return types.SimpleNamespace(**{**hop.__dict__, "s": hop.hrow, "n_old": hop.n_dir * hop.n_old})


def backward(hop, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg, dtype=np.float64):
    """grad_gate [E] (in the hop's edge order), grad_hidden [n_dir * n_old, ld], grad_a_s_dir [n_dir * n_old, ap] in ``dtype``;
    .S / .n per output."""
    a_s_dir = np.repeat(np.asarray(a_s), hop.n_dir, axis=0)
    full = lr.backward(directed_sources(hop), hidden, rela, time_tab, a_s_dir, a_r, a_q, w_alpha, b_alpha, grad_agg, dtype=dtype)
    tabs = (hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg)
    gate = _gate(hop, *lr._cast(np.dtype(dtype), *tabs), absolute=False)
    S = dict(grad_gate=_gate(hop, *lr._cast(np.float64, *tabs), absolute=True), grad_hidden=full.S["grad_hidden"], grad_a_s_dir=full.S["grad_a_s"])
    n = dict(grad_gate=np.ones(hop.E), grad_hidden=full.n["grad_hidden"], grad_a_s_dir=full.n["grad_a_s"])
    return types.SimpleNamespace(grad_gate=gate, grad_hidden=full.grad_hidden, grad_a_s_dir=full.grad_a_s, S=S, n=n)


def group_directions(grad_a_s_dir, n_dir):
    """[n_old, ap]: a source's n_dir rows added in the order past, now, future, as engine.digraph_tlayer_bwd adds them."""
    g = np.asarray(grad_a_s_dir)
    if n_dir == 1:
        return g
    g = g.reshape(-1, 3, g.shape[1])
    return (g[:, 0] + g[:, 1]) + g[:, 2]


def tables(x):
    """The reference's positional arguments from layer_ref.inputs' dict."""
    return tuple(x[k] for k in ("hidden", "rela", "time_tab", "a_s", "a_r", "a_q", "w_alpha", "b_alpha", "grad_agg"))


def take_rows(A, hop, pick):
    """The call that carries only the edges of the directed rows ``pick``, with every table, destination and number as they are (the
    other rows are then empty): (A', at) with ``at`` the kept edges' positions in A's list."""
    at = np.nonzero(np.isin(hop.hrow, pick))[0]
    ptr = np.zeros(len(A["dst_ptr"]), np.int64)
    ptr[1:] = np.cumsum(np.bincount(hop.o[at], minlength=len(A["dst_ptr"]) - 1))
    return dict(dst_ptr=ptr.astype(np.int32), src_idx=A["src_idx"][at], rel=A["rel"][at], row_of_dst=A["row_of_dst"],
                edge_time=A["edge_time"][at]), at


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
N_DIRS = (3, 1)
ROW_WIDTHS = [(16, 16), (20, 32), (64, 64), (20, 128), (16, 256)]
ATTENTION_WIDTHS = [(3, 4), (5, 8), (17, 32)]
HUB_DEGREES = (0, 1, 127, 128, 129, 256, 257, 3000)       # of the DIRECTED rows 0..7; 128: the longest that is not cut; 3000: 24 chunks


def case(name, n_dir, d, ld, attn, ap=None, seed=0):
    """layer_ref's temporal (n_dir 3) or windowed (n_dir 1) case: its default graph, five queries, two hops."""
    make = lr._temporal_case if n_dir == 3 else lr._windowed_case
    c = make(name, seed=seed, d=d, ld=ld, attn_dim=attn, B=5)
    c.n_dir = n_dir
    c.n_tab_rows = c.n_time if n_dir == 3 else c.n_tab          # the kernel's n_time: rows of the time table per direction
    if ap is not None:
        c.ap = ap
    return c


def row_width_case(n_dir, d, ld):
    return case("n_dir%d_d%d_ld%d" % (n_dir, d, ld), n_dir, d, ld, 5, seed=d + ld + n_dir)


def attention_case(n_dir, attn, ap):
    return case("n_dir%d_attn%d_ap%d" % (n_dir, attn, ap), n_dir, 16, 32, attn, ap=ap, seed=attn + ap + n_dir)


def case_hops(c):
    """[(k, hop, A)] of a layer_ref timed case: its oracle hops in destination order (stable), as the kernel's arrays, with the hop
    formed from those arrays (timed_hop); it is layer_ref's own hop_of on the same edges (test_digraph_tbwd_ref.py)."""
    og, nodes, out = lr.oracle_graph(c), c.nodes0, []
    for k in range(c.hops):
        new, edges, etime = lr.expand(c, og, nodes)
        order = np.argsort(edges[:, 5], kind="stable")
        edges, etime = edges[order], np.asarray(etime, np.int64)[order]
        if c.n_dir == 3:
            day = etime                                     # a time id
        else:                                               # the day the caller resolves: the data row's, a self-loop's loop_time
            loop = etime >= c.n_data
            day = np.where(loop, c.loop_time[edges[:, 0]], c.row_time[np.where(loop, 0, etime)])
        ptr = np.zeros(len(new) + 1, np.int64)
        ptr[1:] = np.cumsum(np.bincount(edges[:, 5], minlength=len(new)))
        row_of = np.zeros(len(new), np.int64)
        row_of[edges[:, 5]] = edges[:, 0]
        A = dict(dst_ptr=ptr.astype(np.int32), src_idx=edges[:, 4].astype(np.int32), rel=edges[:, 2].astype(np.int32),
                 row_of_dst=row_of.astype(np.int32), edge_time=day.astype(np.int32))
        hop = timed_hop(A, c.q_time, c.n_dir, len(nodes), c.n_rela_rows, c.n_tab_rows)
        hop.oracle = lr.hop_of(c, edges, etime, len(nodes), len(new))
        out.append((k, hop, A))
        nodes = new
    return out


def hub_hop(n_dir, n_ones=1000, n_dst=300, B=3, seed=43):
    """A hand-built hop whose DIRECTED rows 0..7 have HUB_DEGREES edges, row 8 none, then ``n_ones`` rows of one edge each, into
    ``n_dst`` random destinations of ``B`` rows.  n_dir = 3: source 0 (rows 0, 1, 2) has no past edge and source 2 (rows 6, 7, 8) no
    future edge - edges in exactly two of three directions.  (case, hop, A)."""
    c = case("hub_rows_n_dir%d" % n_dir, n_dir, 20, 32, 5, seed=seed)
    c.B = B
    rng = np.random.default_rng(seed + n_dir)
    deg = np.array(HUB_DEGREES + (0,) + (1,) * n_ones)
    n_old = -(-len(deg) // n_dir)
    u = np.repeat(np.arange(len(deg)), deg)
    E = len(u)
    dst = rng.integers(0, n_dst, E)
    dst[:n_dst] = rng.permutation(n_dst)                   # every destination has an edge
    order = np.lexsort((rng.permutation(E), dst))          # destination order; inside a destination not the source order
    u, dst = u[order], dst[order]
    row_of = rng.integers(0, B, n_dst)
    c.n_tab_rows = 12
    c.q_time = rng.integers(4, 8, B)
    qt = c.q_time[row_of[dst]]
    if n_dir == 3:                                         # the time that puts the edge into its row's direction
        day = qt + (u % 3 - 1) * rng.integers(1, 5, E)
    else:                                                  # lags -2 .. 7: the negative ones clamp to 0 (clamped_hop: past the table)
        day = np.maximum(qt - rng.integers(-2, 16, E), 0)
    ptr = np.zeros(n_dst + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(dst, minlength=n_dst))
    A = dict(dst_ptr=ptr.astype(np.int32), src_idx=(u // n_dir).astype(np.int32), rel=rng.integers(0, c.n_rela_rows, E).astype(np.int32),
             row_of_dst=row_of.astype(np.int32), edge_time=day.astype(np.int32))
    hop = timed_hop(A, c.q_time, n_dir, n_old, c.n_rela_rows, c.n_tab_rows)
    assert np.array_equal(hop.hrow, u)
    return c, hop, A


def clamped_hop(n_dir):
    """Hop 2 of a small case with edge times moved outside the table: n_dir = 3, |dt| >= n_time on both sides; n_dir = 1, a negative
    lag (an edge later than its query) and a lag past the table (day 0 under the latest query).  (case, k, hop, A, moved edges)."""
    c = case("clamped_n_dir%d" % n_dir, n_dir, 20, 32, 5, seed=51)
    k, hop, A = case_hops(c)[1]
    A = dict(A, edge_time=A["edge_time"].copy())
    qt = np.asarray(c.q_time, np.int64)[hop.b]
    n = c.n_tab_rows
    if n_dir == 3:
        at = np.array([0, 1, 2])
        A["edge_time"][at] = (qt[0] + n, qt[1] + n + 7, qt[2] - 3 * n)
    else:
        at = np.array([0 if qt.argmax() else 1, qt.argmax()])
        assert qt[at[1]] >= n + 2
        A["edge_time"][at] = (qt[at[0]] + 5, 0)
    return c, k, timed_hop(A, c.q_time, n_dir, hop.n_old, c.n_rela_rows, n), A, at


def one_edge_hop(n_dir):
    c = case("one_edge_n_dir%d" % n_dir, n_dir, 16, 32, 5, seed=5)
    c.q_time = np.array([3, 9, 4, 4, 4])
    c.n_tab_rows = 12
    A = dict(dst_ptr=np.array([0, 1], np.int32), src_idx=np.array([3], np.int32), rel=np.array([2], np.int32),
             row_of_dst=np.array([1], np.int32), edge_time=np.array([11], np.int32))          # dt = +2: future; lag -2: clamped to 0
    return c, timed_hop(A, c.q_time, n_dir, 4, c.n_rela_rows, c.n_tab_rows), A


def inputs(c, k, hop):
    """layer_ref.inputs for a hop of the case (tables sized by the case, the time table by c.n_tab_rows)."""
    saved = (c.n_time, getattr(c, "n_tab", None))
    c.n_time, c.n_tab = c.n_tab_rows, c.n_tab_rows
    try:
        return lr.inputs(c, k, hop)
    finally:
        c.n_time, c.n_tab = saved


def all_hops():
    """Every (tag, case, k, hop, A) the kernel's tests use."""
    out = []
    for n_dir in N_DIRS:
        cases = [row_width_case(n_dir, d, ld) for d, ld in ROW_WIDTHS] + [attention_case(n_dir, a, ap) for a, ap in ATTENTION_WIDTHS]
        for c in cases:
            out += [("%s hop %d" % (c.name, k + 1), c, k, hop, A) for k, hop, A in case_hops(c)]
        c, hop, A = hub_hop(n_dir)
        out.append((c.name, c, 0, hop, A))
        c, k, hop, A, _ = clamped_hop(n_dir)
        out.append((c.name, c, k, hop, A))
        c, hop, A = one_edge_hop(n_dir)
        out.append((c.name, c, 0, hop, A))
    return out
