"""Per-edge reference of ONE message-passing hop (what include/redgnn.h promises for rg_layer_fwd / rg_layer_bwd, rg_tlayer_* and
rg_xlayer_*), in plain numpy from an explicit edge list, plus the case table the layer-kernel tests share.  TEST INFRASTRUCTURE.

The edge list is the CPU oracle's (oracle.redgnn_oracle.get_neighbors), never the library's: edges int64 [E, 6] =
(batch, head, rel, tail, old_idx, new_idx).  The inputs are the hoisted tables the kernels take (hidden, rela, a_s, a_r, a_q padded to
``ap`` columns with zeros, w_alpha [attn_dim], b_alpha [1], grad_agg).

    per edge e = (b, s, r, o):   z = relu(a_s[s] + a_r[r] + a_q[b]);   alpha = sigmoid(w . z + b_alpha)
      static     m = hidden[s] + rela[r]
      temporal   m = hidden_dir[3 s + dir] + rela_dir[dir * n_rela_rows + r] + time_dir[dir * n_time + |dt|],  dt = time(e) - q_time[b],
                 dir = 0 (dt < 0) / 1 (dt = 0) / 2 (dt > 0)
      windowed   m = hidden_p[s] + rela_p[r] + time_p[trow],  trow = clamp(q_time[b] - row_time[row(e)], 0, n_tab - 1)
                 (self-loops, row >= n_data: q_time[b] - loop_time[b]); an edge exists for query b iff row in [win_lo[b], win_hi[b]) or
                 row >= n_data
    forward    agg[o] = sum_e alpha_e m_e
    backward   g_alpha = <G[o], m>;  g_p = g_alpha alpha (1 - alpha);  g_z = g_p w 1[z > 0]        (G = grad_agg)
               grad_hidden[row of s] += alpha G[o];  grad_rela[row of r] += alpha G[o];  grad_time[trow] += alpha G[o]
               grad_a_s[s] += g_z;  grad_a_r[r] += g_z;  grad_a_q[b] += g_z;  grad_w_alpha += g_p z;  grad_b_alpha += g_p

Every function takes ``dtype``: np.float64 is the reference; np.float32 (the same code in the same edge order) is the yardstick of
what a correct fp32 evaluation costs.  Besides each output the functions return, in fp64, ``n`` = the number of edges summed into the
element and ``S`` = the same sum with every term replaced by its absolute value: |hidden| + |rela| (+ |time|) for m, |G| for G,
|G| . (|hidden| + |rela| + ...) for g_alpha, |w| for w.  The same rule is applied to the sum INSIDE the sigmoid, carried through it to
first order: with Z = |b_alpha| + sum_j |w_j| (|a_s| + |a_r| + |a_q|)_j (the absolute form of w . z + b_alpha, what the rounding error of
that sum and of the exp's argument scale with) and d alpha / d z = alpha (1 - alpha),

    alpha            -> kappa = alpha + alpha (1 - alpha) Z
    alpha (1 - alpha) -> kappa as well:  alpha (1 - alpha) + alpha^2 (1 - alpha is formed from a rounded alpha: error u alpha, times
                         alpha) + alpha (1 - alpha) |1 - 2 alpha| Z  <=  kappa

Without that term the bound is not satisfiable by ANY fp32 evaluation where the attention saturates (w_alpha x 50: Z ~ 10^3, and
1 - alpha cancels): the plain-numpy fp32 run of this file then misses it by factors of 10^4 .. 10^6 (measured).  The error of an fp32
sum scales with u * S:

    |fp32 - fp64| <= c * (n + n0) * u * S + tiny         u = 2^-24, tiny = 1e-30 (S = 0: the value must be exactly 0)

n0 (``n0_of``) is the per-term work: attn_dim fused multiply-adds of the attention dot product, the two adds of a_s + a_r + a_q, exp and
reciprocal (1 ulp each on the device), the add(s) forming m and the product alpha * m: attn_dim + 6.  The attention gradients go
through g_alpha, a dot product of d terms, then alpha (1 - alpha) and w: + d + 3.  ``C_BOUND`` below is 4 x the worst ratio
|ref32 - ref64| / ((n + n0) u S) measured over every element of every output of every case of the table (test_layer_ref.py keeps
that measurement honest: it fails if a case exceeds REF32_WORST_RATIO).
"""
import types

import numpy as np

from oracle import redgnn_oracle as orc

U = 2.0 ** -24
TINY = 1e-30
# measured: max over all cases, hops, outputs and elements of |ref32 - ref64| / ((n + n0) * u * S)  (test_fp32_reference_within_its_bound
# prints the per-case figures); rounded up
REF32_WORST_RATIO = 0.4
# the GPU's allowance: 4 x the fp32 reference's own cost (another summation order - segments of 128, partial rows, float atomics - and the
# 1-ulp hardware exp / reciprocal); the factor tests/_util.assert_close_fp32 grants the GPU over the CPU fp32 path
C_BOUND = 4.0 * REF32_WORST_RATIO

FWD_OUTPUTS = ("agg",)
BWD_OUTPUTS = ("grad_hidden", "grad_rela", "grad_time", "grad_a_s", "grad_a_r", "grad_a_q", "grad_w_alpha", "grad_b_alpha")
_ATTN = ("grad_a_s", "grad_a_r", "grad_a_q", "grad_w_alpha", "grad_b_alpha")


def n0_of(name, d, attn_dim):
    return attn_dim + 6 + (d + 3 if name in _ATTN else 0)


def bound(S, n, n0, c):
    return c * (np.asarray(n, np.float64) + n0) * U * np.asarray(S, np.float64) + TINY


# ---- a hop as index arrays ----------------------------------------------------------------------------------------------------
def static_hop(edges, n_old, n_new):
    e = np.asarray(edges, np.int64)
    return types.SimpleNamespace(kind="static", b=e[:, 0], s=e[:, 4], r=e[:, 2], o=e[:, 5], hrow=e[:, 4], rrow=e[:, 2], trow=None,
                                 n_old=int(n_old), n_new=int(n_new), E=len(e))


def temporal_hop(edges, etime, q_time, n_old, n_new, n_rela_rows, n_time):
    e = np.asarray(edges, np.int64)
    dt = np.asarray(etime, np.int64) - np.asarray(q_time, np.int64)[e[:, 0]]
    dirn = np.where(dt > 0, 2, np.where(dt == 0, 1, 0))
    return types.SimpleNamespace(kind="temporal", b=e[:, 0], s=e[:, 4], r=e[:, 2], o=e[:, 5], hrow=3 * e[:, 4] + dirn,
                                 rrow=dirn * n_rela_rows + e[:, 2], trow=dirn * n_time + np.abs(dt), n_old=int(n_old), n_new=int(n_new),
                                 E=len(e), dir=dirn, dt=dt)


def window_valid(edges, erow, win_lo, win_hi, n_data):
    """Which edges exist for their query: data row inside the query's window, or a self-loop (row >= n_data)."""
    b = np.asarray(edges, np.int64)[:, 0]
    erow = np.asarray(erow, np.int64)
    return (erow >= n_data) | ((erow >= np.asarray(win_lo, np.int64)[b]) & (erow < np.asarray(win_hi, np.int64)[b]))


def windowed_hop(edges, erow, q_time, loop_time, row_time, n_data, n_tab, n_old, n_new):
    """edges: already restricted to the valid ones (window_valid) with new_idx numbered over their tails."""
    e = np.asarray(edges, np.int64)
    erow = np.asarray(erow, np.int64)
    b = e[:, 0]
    loop = erow >= n_data
    t_e = np.where(loop, np.asarray(loop_time, np.int64)[b], np.asarray(row_time, np.int64)[np.where(loop, 0, erow)])
    trow = np.clip(np.asarray(q_time, np.int64)[b] - t_e, 0, n_tab - 1)
    return types.SimpleNamespace(kind="windowed", b=b, s=e[:, 4], r=e[:, 2], o=e[:, 5], hrow=e[:, 4], rrow=e[:, 2], trow=trow,
                                 n_old=int(n_old), n_new=int(n_new), E=len(e))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------
def _scatter(idx, vals, n_rows):
    """out[idx[e]] += vals[e] in edge order (np.add.at; element-wise over the row so the 1-D fast path applies)."""
    vals = np.ascontiguousarray(vals)
    if vals.ndim == 1:
        out = np.zeros(n_rows, vals.dtype)
        np.add.at(out, idx, vals)
        return out
    cols = vals.shape[1]
    out = np.zeros(n_rows * cols, vals.dtype)
    np.add.at(out, (np.asarray(idx, np.int64)[:, None] * cols + np.arange(cols)).ravel(), vals.ravel())
    return out.reshape(n_rows, cols)


def _cast(dt, *xs):
    return [None if x is None else np.asarray(x).astype(dt) for x in xs]


def _attention(hop, a_s, a_r, a_q, w_alpha, b_alpha):
    dt = a_s.dtype
    w = np.zeros(a_s.shape[1], dt)
    w[:len(w_alpha)] = w_alpha
    zr = np.maximum(a_s[hop.s] + a_r[hop.r] + a_q[hop.b], dt.type(0))
    z = (zr * w).sum(1, dtype=dt) + b_alpha.reshape(-1)[0]
    with np.errstate(over="ignore"):      # exp(-z) = inf: alpha = 0, as on the device
        alpha = dt.type(1) / (dt.type(1) + np.exp(-z))
    return w, zr, alpha


def _kappa(hop, a_s, a_r, a_q, w_alpha, b_alpha, alpha):
    """alpha + alpha (1 - alpha) Z: the absolute-value form of alpha (and of alpha (1 - alpha)), see the module docstring."""
    w = np.zeros(a_s.shape[1], a_s.dtype)
    w[:len(w_alpha)] = np.abs(w_alpha)
    Z = ((np.abs(a_s[hop.s]) + np.abs(a_r[hop.r]) + np.abs(a_q[hop.b])) * w).sum(1) + np.abs(b_alpha.reshape(-1)[0])
    return alpha + alpha * (1 - alpha) * Z


kappa = _kappa      # (public: tests/hop_ref.py bounds a single alpha with it)


def _message(hop, hidden, rela, time_tab, absolute=False):
    f = np.abs if absolute else (lambda x: x)
    m = f(hidden[hop.hrow]) + f(rela[hop.rrow])
    if hop.trow is not None:
        m = m + f(time_tab[hop.trow])
    return m


def forward(hop, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, dtype=np.float64):
    """agg [n_new, ld], alpha [E] in ``dtype``; S["agg"], n["agg"] in fp64 / counts."""
    dt = np.dtype(dtype)
    h, r, t, as_, ar, aq, w, b = _cast(dt, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha)
    _, _, alpha = _attention(hop, as_, ar, aq, w, b)
    agg = _scatter(hop.o, alpha[:, None] * _message(hop, h, r, t), hop.n_new)
    h, r, t, as_, ar, aq, w, b = _cast(np.float64, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha)
    _, _, alpha64 = _attention(hop, as_, ar, aq, w, b)
    S = _scatter(hop.o, _kappa(hop, as_, ar, aq, w, b, alpha64)[:, None] * _message(hop, h, r, t, absolute=True), hop.n_new)
    n = np.bincount(hop.o, minlength=hop.n_new)[:, None]
    return types.SimpleNamespace(agg=agg, alpha=alpha, S=dict(agg=S), n=dict(agg=n))


def _backward_values(hop, B, h, r, t, as_, ar, aq, w_alpha, b, G_rows, absolute):
    """The seven (eight with the time table) sums; absolute = the S form (every term replaced by its absolute value)."""
    w, zr, alpha = _attention(hop, as_, ar, aq, w_alpha, b)
    G = G_rows[hop.o]
    if absolute:
        G, w = np.abs(G), np.abs(w)
        alpha = _kappa(hop, as_, ar, aq, w_alpha, b, alpha)
        zr = (np.abs(as_[hop.s]) + np.abs(ar[hop.r]) + np.abs(aq[hop.b])) * (zr > 0)
    m = _message(hop, h, r, t, absolute)
    g_alpha = (G * m).sum(1, dtype=G.dtype)
    g_p = g_alpha * alpha if absolute else g_alpha * alpha * (G.dtype.type(1) - alpha)
    g_z = g_p[:, None] * w[None, :] * (zr > 0)
    aG = alpha[:, None] * G
    out = dict(grad_hidden=_scatter(hop.hrow, aG, h.shape[0]), grad_rela=_scatter(hop.rrow, aG, r.shape[0]),
               grad_time=None if hop.trow is None else _scatter(hop.trow, aG, t.shape[0]),
               grad_a_s=_scatter(hop.s, g_z, hop.n_old), grad_a_r=_scatter(hop.r, g_z, ar.shape[0]), grad_a_q=_scatter(hop.b, g_z, B),
               grad_w_alpha=(g_p[:, None] * zr).sum(0, dtype=G.dtype)[:len(w_alpha)] if hop.E else np.zeros(len(w_alpha), G.dtype),
               grad_b_alpha=g_p.sum(dtype=G.dtype).reshape(1))
    return out


def backward(hop, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg, dtype=np.float64):
    """grad_hidden (shape of hidden: the temporal form's rows 3 s + dir), grad_rela, grad_time (None for the static layer), grad_a_s
    [n_old, ap], grad_a_r, grad_a_q [B, ap], grad_w_alpha [attn_dim], grad_b_alpha [1] in ``dtype``; .S / .n per output name."""
    B = np.asarray(a_q).shape[0]
    dt = np.dtype(dtype)
    vals = _backward_values(hop, B, *_cast(dt, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg), absolute=False)
    S = _backward_values(hop, B, *_cast(np.float64, hidden, rela, time_tab, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg), absolute=True)
    cnt = lambda idx, rows: np.bincount(idx, minlength=rows)[:, None]
    n = dict(grad_hidden=cnt(hop.hrow, np.asarray(hidden).shape[0]), grad_rela=cnt(hop.rrow, np.asarray(rela).shape[0]),
             grad_time=None if hop.trow is None else cnt(hop.trow, np.asarray(time_tab).shape[0]),
             grad_a_s=cnt(hop.s, hop.n_old), grad_a_r=cnt(hop.r, np.asarray(a_r).shape[0]), grad_a_q=cnt(hop.b, B),
             grad_w_alpha=hop.E, grad_b_alpha=hop.E)
    return types.SimpleNamespace(S=S, n=n, **vals)


def worst_ratio(val, ref, S, n, n0):
    """max (|val - ref| - tiny) / ((n + n0) u S) over the elements: the c that ``bound`` would need (errors below tiny count as 0, fp32
    underflow of alpha ~ 1e-40 among them; inf where S = 0 and the values differ by more than tiny)."""
    err = np.maximum(np.abs(np.asarray(val, np.float64) - np.asarray(ref, np.float64)) - TINY, 0.0)
    den = (np.asarray(n, np.float64) + n0) * U * np.asarray(S, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(den > 0, err / den, np.where(err > 0, np.inf, 0.0))
    return float(q.max())


# ---- oracle edge lists ------------------------------------------------------------------------------------------------------------
def quad_graph(quads, n_ent, n_rela_rows):
    """A graph get_neighbors can walk whose rows are the quadruples as given (no inverse / identity rows added): its edges then
    carry the time field as a fifth column."""
    g = orc.OracleGraph.__new__(orc.OracleGraph)
    g.KG = np.asarray(quads, np.int64).reshape(-1, 4)
    g.n_fact, g.n_ent, g.n_rel = len(g.KG), n_ent, (n_rela_rows - 1) // 2
    g.rows_by_head = np.argsort(g.KG[:, 0], kind="stable")
    ptr = np.zeros(n_ent + 1, np.int64)
    np.add.at(ptr, g.KG[:, 0] + 1, 1)
    g.head_ptr = np.cumsum(ptr)
    return g


def expand(case, og, nodes):
    """One hop from ``nodes`` (int64 [N, 2], sorted): (new nodes, edges [E, 6], edge time field or None), all from the oracle."""
    new, edges, _ = orc.get_neighbors(og, nodes)
    if case.kind == "static":
        return new, edges, None
    etime, edges = edges[:, 4], np.concatenate([edges[:, :4], edges[:, 5:7]], 1)
    if case.kind == "windowed":
        keep = window_valid(edges, etime, case.win_lo, case.win_hi, case.n_data)
        edges, etime = edges[keep], etime[keep]
        key = edges[:, 0] * case.n_ent + edges[:, 3]
        uk, inv = np.unique(key, return_inverse=True)
        new = np.stack([uk // case.n_ent, uk % case.n_ent], 1)
        edges = np.concatenate([edges[:, :5], inv.reshape(-1, 1)], 1)
    return new, edges, etime


def hop_of(case, edges, etime, n_old, n_new):
    if case.kind == "static":
        return static_hop(edges, n_old, n_new)
    if case.kind == "temporal":
        return temporal_hop(edges, etime, case.q_time, n_old, n_new, case.n_rela_rows, case.n_time)
    return windowed_hop(edges, etime, case.q_time, case.loop_time, case.row_time, case.n_data, case.n_tab, n_old, n_new)


def oracle_graph(case):
    if case.kind == "static":
        return orc.OracleGraph(orc.double_triple(case.triples, case.n_rel), case.n_ent, case.n_rel)
    return quad_graph(case.quads, case.n_ent, case.n_rela_rows)


def hops(case):
    """[(nodes_old, nodes_new, edges, hop)] of the case's hops, from the CPU oracle."""
    og, nodes, out = oracle_graph(case), case.nodes0, []
    for _ in range(case.hops):
        new, edges, etime = expand(case, og, nodes)
        out.append((nodes, new, edges, hop_of(case, edges, etime, len(nodes), len(new))))
        nodes = new
    return out


def inputs(case, k, hop):
    """Seeded random inputs of hop k: dict of float32 arrays in the kernels' layouts (pad columns of hidden / rela / a_* zero)."""
    rng = np.random.default_rng(1000 + 17 * k + case.seed)
    d, ld, attn, ap = case.d, case.ld, case.attn_dim, case.ap
    nd = 3 if case.kind == "temporal" else 1

    def table(rows, cols, used, scale=1.0):
        x = np.zeros((rows, cols), np.float32)
        x[:, :used] = rng.standard_normal((rows, used)) * scale
        return x
    x = dict(hidden=table(nd * hop.n_old, ld, d), rela=table(nd * case.n_rela_rows, ld, d),
             time_tab=None if case.kind == "static" else table(nd * case.n_time if case.kind == "temporal" else case.n_tab, ld, d),
             a_s=table(hop.n_old, ap, attn), a_r=table(case.n_rela_rows, ap, attn), a_q=table(case.B, ap, attn),
             w_alpha=rng.standard_normal(attn).astype(np.float32), b_alpha=rng.standard_normal(1).astype(np.float32) * 0.5,
             grad_agg=rng.standard_normal((hop.n_new, ld)).astype(np.float32))
    if case.kind != "static":
        x["b_alpha"][:] = 0      # the temporal attention has no bias (redgnn.h: pass b_alpha = 0)
    if case.regime == "saturated":      # alpha within 1e-6 of 0 or 1, g_p ~ 0
        x["w_alpha"] *= 50
    elif case.regime == "dead":         # z = 0 everywhere: alpha = sigmoid(b_alpha), g_z = 0 exactly
        x["a_q"][:, :attn] = -100
    return x


# ---- the case table -----------------------------------------------------------------------------------------------------------------
# Every case names the host-side condition it is built to flip.  Defaults: ld 64, attn_dim 5, packed entries, static, B = 33, two hops
# from one subject per query (hop 1: sparse walks, hop 2: dense walks).
def _rand_triples(rng, n_ent, n_rel, m, hub=True, isolated=1):
    """m random triples over entities 0 .. n_ent - 1 - isolated (the last ``isolated`` entities keep only their identity edge); with
    ``hub`` one entity is the tail of a tenth of them and another the head of a tenth; seven triples are duplicated."""
    top = n_ent - isolated
    h, t = rng.integers(0, top, m), rng.integers(0, top, m)
    if hub:
        t[: m // 10] = 3 % top
        h[m // 10: m // 5] = 5 % top
    trip = np.stack([h, rng.integers(0, n_rel, m), t], 1)
    return np.concatenate([trip, trip[:7]], 0)


def _subjects(rng, B, n_ent, first=None):
    sub = rng.integers(0, n_ent, B)
    if first is not None:
        sub[0] = first
    return np.stack([np.arange(B), sub], 1).astype(np.int64)


def _pad_attn(attn_dim):
    """The padded attention width the kernels are compiled for (common.h with_ap4): a multiple of 4 up to 16, then 32."""
    ap = (attn_dim + 3) // 4 * 4
    return ap if ap <= 16 else 32


def _case(name, seed=0, kind="static", n_ent=200, n_rel=5, m=1500, B=33, hops=2, d=64, ld=None, attn_dim=5, regime="generic",
          triples=None, nodes0=None, **extra):
    rng = np.random.default_rng(seed + 7)
    ld = d if ld is None else ld
    c = types.SimpleNamespace(name=name, seed=seed, kind=kind, n_ent=n_ent, n_rel=n_rel, B=B, hops=hops, d=d, ld=ld, attn_dim=attn_dim,
                              ap=_pad_attn(attn_dim), regime=regime, n_rela_rows=2 * n_rel + 1, reset="nodes" if nodes0 is not None else "subjects")
    c.triples = _rand_triples(rng, n_ent, n_rel, m) if triples is None else np.asarray(triples, np.int64)
    # query 0 starts from an entity that has only its identity edge
    c.nodes0 = _subjects(rng, B, n_ent, first=n_ent - 1 if triples is None else None) if nodes0 is None else np.asarray(nodes0, np.int64)
    for k, v in extra.items():
        setattr(c, k, v)
    return c


def _hub_case(name):
    """Segment cuts (RG_VROW_MAX = 128, common.h): entities of in- and out-degree 1, 127, 128, 129, 256, 257 and 3000 (identity edge
    included), every neighbour a leaf of its own; the last two triples of a hub duplicate its first two (parallel edges count twice).
    Query 0 starts from every entity, query 1 from the hubs only (hub = source: the backward's g_hidden_part / g_as_part), query 2 from
    the leaves only (hub = destination only: the forward's partial rows)."""
    degs = [1, 127, 128, 129, 256, 257, 3000]
    trip, nxt = [], len(degs)
    for i, k in enumerate(degs):
        rows = []
        for j in range(max(k - 1 - 2, 0) if k > 3 else k - 1):
            rows.append((i, j % 3, nxt) if j % 2 else (nxt, j % 3, i))
            nxt += 1
        if k > 3:
            rows += rows[:2]
        trip += rows
    n_ent = nxt
    ent = np.arange(n_ent)
    z = lambda b, e: np.stack([np.full(len(e), b), e], 1)
    nodes0 = np.concatenate([z(0, ent), z(1, ent[:len(degs)]), z(2, ent[len(degs):])], 0)
    return _case(name, seed=31, n_ent=n_ent, n_rel=3, B=3, hops=1, triples=trip, nodes0=nodes0)


def _wide_ent_triples(rng, n_ent, n_rel, m):
    """~m triples over a few hundred entities at both ends of the id range (so two hops stay small), the highest ids in use."""
    pool = np.concatenate([np.arange(150), n_ent - 1 - np.arange(150)])
    h, t = pool[rng.integers(0, 300, m)], pool[rng.integers(0, 300, m)]
    h[:5], t[:5] = n_ent - 1, n_ent - 2 - np.arange(5)
    t[5:10], h[5:10] = n_ent - 1, np.arange(5)
    return np.stack([h, rng.integers(0, n_rel, m), t], 1)


def _wide_ent_case(name, n_ent, ld, seed, kind="static"):
    rng = np.random.default_rng(seed)
    trip = _wide_ent_triples(rng, n_ent, 5, 5000)
    nodes0 = np.stack([np.arange(3), [n_ent - 1, 7, n_ent - 3]], 1)
    if kind == "static":
        return _case(name, seed=seed, n_ent=n_ent, n_rel=5, B=3, d=ld, triples=trip, nodes0=nodes0)
    return _temporal_case(name, seed=seed, n_ent=n_ent, B=3, d=ld, triples=trip, nodes0=nodes0)


def _wide_rel_case(name, n_rel, ld, seed, kind="static", ident_ent=None):
    """n_rel = 2050: 4101 relation rows (> 2^12: int2 entries; the attention table alone passes 64 KiB of LDS, attn_dim <= 4 keeps it
    under 160 KiB).  n_rel = 2047: 4095 rows, still packed, identity relation 4094."""
    rng = np.random.default_rng(seed)
    n_ent = 300
    trip = _rand_triples(rng, n_ent, n_rel, 1500)
    trip[:4, 1] = n_rel - 1
    if kind == "static":
        return _case(name, seed=seed, n_ent=n_ent, n_rel=n_rel, B=3, d=ld, attn_dim=4, triples=trip,
                     nodes0=_subjects(rng, 3, n_ent, first=n_ent - 1))
    return _temporal_case(name, seed=seed, n_ent=n_ent, n_rel=n_rel, B=3, d=ld, attn_dim=4, triples=trip,
                          nodes0=_subjects(rng, 3, n_ent, first=n_ent - 1))


def _temporal_case(name, seed=0, n_ent=200, n_rel=5, m=1500, B=33, n_time=12, triples=None, nodes0=None, **kw):
    """T-RED-GNN interpolation: quadruples (h, r, t, time) with their inverses and one identity row per entity (relation 2 n_rel,
    time n_time - 1), used as given.  Query times cover 0 and n_time - 1, so dt < 0, = 0, > 0 and |dt| = n_time - 1 all occur."""
    rng = np.random.default_rng(seed + 11)
    c = _case(name, seed=seed, kind="temporal", n_ent=n_ent, n_rel=n_rel, m=m, B=B, triples=triples, nodes0=nodes0, **kw)
    tr = c.triples
    tm = rng.integers(0, n_time, len(tr))
    tm[:3] = (0, n_time - 1, n_time // 2)
    ent = np.arange(n_ent)
    c.quads = np.concatenate([np.column_stack([tr, tm]), np.column_stack([tr[:, 2], tr[:, 1] + n_rel, tr[:, 0], tm]),
                              np.column_stack([ent, np.full(n_ent, 2 * n_rel), ent, np.full(n_ent, n_time - 1)])], 0).astype(np.int64)
    c.n_time = n_time
    c.q_time = rng.integers(0, n_time, B)
    c.q_time[:min(B, 3)] = (0, n_time - 1, n_time // 2)[:min(B, 3)]
    return c


def _windowed_case(name, seed=0, n_ent=200, n_rel=5, m=1500, B=33, n_days=20, n_tab=6, **kw):
    """Temporal extrapolation: data rows sorted by day; the graph's time field is the data row (self-loops: n_data).  Query 0: empty
    window; query 1: every row (rows of later days too: delta < 0 clamps to 0); query 2: older than the first row (day 0, empty window);
    query 3: a subject with nothing but its self-loop; the others see the rows of the days before their own, at most 15 back, so
    delta reaches past n_tab - 1 and clamps there."""
    rng = np.random.default_rng(seed + 13)
    c = _case(name, seed=seed, kind="windowed", n_ent=n_ent, n_rel=n_rel, m=m, B=B, **kw)
    tr = np.concatenate([c.triples, np.column_stack([c.triples[:, 2], c.triples[:, 1] + n_rel, c.triples[:, 0]])], 0)
    day = np.sort(rng.integers(0, n_days, len(tr)))
    tr = tr[rng.permutation(len(tr))]
    c.n_data, c.n_time, c.n_tab = len(tr), len(tr) + 1, n_tab
    ent = np.arange(n_ent)
    c.quads = np.concatenate([np.column_stack([tr, np.arange(len(tr))]),
                              np.column_stack([ent, np.full(n_ent, 2 * n_rel), ent, np.full(n_ent, c.n_data)])], 0).astype(np.int64)
    c.row_time = day.astype(np.int64)
    c.q_time = rng.integers(1, n_days + 3, B)
    begin = np.maximum(c.q_time - 15, 0)
    c.win_lo, c.win_hi = np.searchsorted(day, begin), np.searchsorted(day, c.q_time)
    c.loop_time = begin.copy()
    c.win_lo[0] = c.win_hi[0] = c.n_data // 2
    c.win_lo[1], c.win_hi[1], c.q_time[1] = 0, c.n_data, n_days // 2
    c.q_time[2], c.win_lo[2], c.win_hi[2], c.loop_time[2] = 0, 0, 0, 0
    c.nodes0[3, 1] = n_ent - 1
    return c


def _dense_start(rng, B, n_ent, frac):
    """Level 0 = a random ``frac`` of all entities per query (rg_frontier_reset_nodes), sorted by (query, entity)."""
    return np.concatenate([np.stack([np.full(int(n_ent * frac), b), np.sort(rng.choice(n_ent, int(n_ent * frac), replace=False))], 1)
                           for b in range(B)], 0)


CASES = {
    "default": lambda: _case("default"),
    # ---- lane group G (common.h with_g: the power of two >= ld / 4): 4, 8, 16 (default and d 48), 32, 64; d < ld: pad columns
    "g4_ld16": lambda: _case("g4_ld16", seed=1, d=16),
    "g8_ld20": lambda: _case("g8_ld20", seed=2, d=20),
    "g8_ld32": lambda: _case("g8_ld32", seed=3, d=32),
    "g8_d30_ld32": lambda: _case("g8_d30_ld32", seed=4, d=30, ld=32),
    "g16_ld48": lambda: _case("g16_ld48", seed=5, d=48),
    "g32_ld128": lambda: _case("g32_ld128", seed=6, d=128, B=9),
    "g64_ld256": lambda: _case("g64_ld256", seed=7, d=256, B=5),
    # ---- AP4 (common.h with_ap4: ap / 4 in {1, 2, 3, 4, 8}); attn_dim % 4 != 0: pad columns of a_*
    "ap_1": lambda: _case("ap_1", seed=8, attn_dim=1),
    "ap_3": lambda: _case("ap_3", seed=9, attn_dim=3),
    "ap_4": lambda: _case("ap_4", seed=10, attn_dim=4),
    "ap_12": lambda: _case("ap_12", seed=11, attn_dim=12),
    "ap_16": lambda: _case("ap_16", seed=12, attn_dim=16),
    "ap_17": lambda: _case("ap_17", seed=13, attn_dim=17, B=9),
    "ap_32": lambda: _case("ap_32", seed=14, attn_dim=32, B=9),
    # ---- PACKED = false (graph.hip build_graph: packed entries iff n_ent <= 2^20 && n_rela_rows <= 2^12), G = 16 and 32
    "wide_ent_ld64": lambda: _wide_ent_case("wide_ent_ld64", (1 << 20) + 37, 64, 15),
    "wide_ent_ld128": lambda: _wide_ent_case("wide_ent_ld128", (1 << 20) + 37, 128, 16),
    "wide_rel_ld64": lambda: _wide_rel_case("wide_rel_ld64", 2050, 64, 17),
    "wide_rel_ld128": lambda: _wide_rel_case("wide_rel_ld128", 2050, 128, 18),
    "t_wide_ent_ld64": lambda: _wide_ent_case("t_wide_ent_ld64", (1 << 20) + 37, 64, 19, kind="temporal"),
    "t_wide_ent_ld128": lambda: _wide_ent_case("t_wide_ent_ld128", (1 << 20) + 37, 128, 20, kind="temporal"),
    "t_wide_rel_ld64": lambda: _wide_rel_case("t_wide_rel_ld64", 2050, 64, 21, kind="temporal"),
    # ---- the boundaries that stay packed: entity 2^20 - 1 as head and as tail; 4095 relation rows, identity relation 4094
    "ent_2p20": lambda: _wide_ent_case("ent_2p20", 1 << 20, 64, 22),
    "rel_4095": lambda: _wide_rel_case("rel_4095", 2047, 64, 23),
    # ---- KPG (walk.h walk_kpg: n_fact / n_vrows < 12 -> 8 items per lane group of the dense walk); dense from level 0 on
    "short_rows_dense": lambda: _case("short_rows_dense", seed=24, n_ent=1000, m=1500, B=5, hops=1,
                                      nodes0=_dense_start(np.random.default_rng(24), 5, 1000, 0.4),
                                      triples=_rand_triples(np.random.default_rng(24), 1000, 5, 1500, hub=False)),
    # ---- RELA_LDS = false (layer_fwd_kernel.h launch2k: lds + rela_bytes <= 53 KiB; layer_bwd_kernel.h launch2: <= 80 KiB) and
    # drel TABLE = false (layer_bwd.hip launch_drel: lds + table <= 80 KiB): 475 relation rows at ld 128.  The other static cases
    # (11 rows) have both in LDS.
    "rela_global": lambda: _case("rela_global", seed=25, n_rel=237, d=128, B=9),
    # ---- segment cuts
    "hubs": lambda: _hub_case("hubs"),
    # ---- batch / bitmap words: B around 32 and 64, n_ent around a bitmap word
    "b1_e33": lambda: _case("b1_e33", seed=26, B=1, n_ent=33, m=120),
    "b31_e97": lambda: _case("b31_e97", seed=27, B=31, n_ent=97, m=400),
    "b32_e1000": lambda: _case("b32_e1000", seed=28, B=32, n_ent=1000, m=3000),
    "b65_e97": lambda: _case("b65_e97", seed=29, B=65, n_ent=97, m=400),
    "b33_e1000": lambda: _case("b33_e1000", seed=30, B=33, n_ent=1000, m=3000),
    # ---- tickets of more than one item in the word-parallel walk (layer_fwd.hip wp_tickets: items per ticket = min(200 n_items / E,
    # n_items / 8192, 32), n_items = BW * n_sub * n_packs: every other case has n_items < 8192, i.e. 1): BW = 32 and >= 317 packs allow
    # 1, 2, 4, 9, 19 (or more) on walks 2 .. 6 and reach the cap of 32 at walk 7 (>= 324 k items; layer_fwd_wp.hip resolve: the partial tail
    # ticket, launch4: the grid).  B * W = 16384 frontier words > SMALL_MAX_WORDS (frontier.hip enqueue_expand: the general level build).
    # One hop (n_new 65931, E 82760); the d 48 twin runs launch3's non-EXACT instance
    "tickets": lambda: _case("tickets", seed=41, n_ent=500, n_rel=5, m=20000, B=1024, hops=1, d=64),
    "tickets_d48": lambda: _case("tickets_d48", seed=41, n_ent=500, n_rel=5, m=20000, B=1024, hops=1, d=48),
    # ---- layer kind
    "temporal": lambda: _temporal_case("temporal", seed=32),
    "windowed": lambda: _windowed_case("windowed", seed=33),
    # ---- attention regime
    "saturated": lambda: _case("saturated", seed=34, regime="saturated"),
    "dead": lambda: _case("dead", seed=35, regime="dead"),
}
