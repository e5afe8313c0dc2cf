"""Per-edge reference of rg_digraph_layer_bwd - the adjoint of ONE rg_digraph_layer_fwd hop (static form) with respect to a gate on
every edge's message, the source states and their attention projection - in plain numpy, fp64 and fp32, and the cases the kernel's
tests share.  TEST INFRASTRUCTURE.

grad_hidden and grad_a_s are tests/layer_ref.backward's, with its S, n and n0 unchanged.  grad_gate is added here under the rule that
file's docstring states: per edge e = (b, s, r, o), G = grad_agg,

    grad_gate[e] = alpha_e * <G[o], hidden[s] + rela[r]>
    S            = kappa_e * sum_j |G[o]_j| (|hidden[s]_j| + |rela[r]_j|)       kappa = alpha + alpha (1 - alpha) Z, the absolute form of alpha
    n            = 1                                                            one term per element
    n0           = attn_dim + 6 + d                                             the attention's work, then a dot product of d terms

Measured over every case below (test_digraph_bwd_ref.py prints the per-case figures): the fp32 run of this file stays within
|ref32 - ref64| / ((n + n0) u S) <= 0.07 for grad_gate (0.15 for grad_hidden, 0.015 for grad_a_s), under layer_ref.REF32_WORST_RATIO =
0.4: the model holds for grad_gate as stated; C_BOUND is layer_ref's, unchanged.
"""
import types

import numpy as np

from tests import layer_ref as lr

OUTPUTS = ("grad_gate", "grad_hidden", "grad_a_s")


def n0_of(name, d, attn_dim):
    return attn_dim + 6 + d if name == "grad_gate" else lr.n0_of(name, d, attn_dim)


def _gate(hop, hidden, rela, a_s, a_r, a_q, w_alpha, b_alpha, G_rows, absolute):
    _, _, alpha = lr._attention(hop, a_s, a_r, a_q, w_alpha, b_alpha)
    G = G_rows[hop.o]
    if absolute:
        G, alpha = np.abs(G), lr._kappa(hop, a_s, a_r, a_q, w_alpha, b_alpha, alpha)
    return alpha * (G * lr._message(hop, hidden, rela, None, absolute)).sum(1, dtype=G.dtype)


def backward(hop, hidden, rela, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg, dtype=np.float64):
    """grad_gate [E] (in the hop's edge order), grad_hidden [n_old, ld], grad_a_s [n_old, ap] in ``dtype``; .S / .n per output."""
    full = lr.backward(hop, hidden, rela, None, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg, dtype=dtype)
    tabs = (hidden, rela, a_s, a_r, a_q, w_alpha, b_alpha, grad_agg)
    gate = _gate(hop, *lr._cast(np.dtype(dtype), *tabs), absolute=False)
    S = dict(grad_gate=_gate(hop, *lr._cast(np.float64, *tabs), absolute=True), grad_hidden=full.S["grad_hidden"], grad_a_s=full.S["grad_a_s"])
    n = dict(grad_gate=np.ones(hop.E), grad_hidden=full.n["grad_hidden"], grad_a_s=full.n["grad_a_s"])
    return types.SimpleNamespace(grad_gate=gate, grad_hidden=full.grad_hidden, grad_a_s=full.grad_a_s, S=S, n=n)


# ---- a hop as the kernel's arrays --------------------------------------------------------------------------------------------------
def by_destination(edges, n_old, n_new):
    """The oracle's hop edges (batch, head, rel, tail, old_idx, new_idx) in destination order (stable), as a layer_ref hop plus the
    forward's arrays (dst_ptr, src_idx, rel, row_of_dst) in numpy: what tests/test_digraph_layer_gpu.py hands rg_digraph_layer_fwd."""
    e = np.asarray(edges, np.int64)
    e = e[np.argsort(e[:, 5], kind="stable")]
    hop = lr.static_hop(e, n_old, n_new)
    ptr = np.zeros(n_new + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(e[:, 5], minlength=n_new))
    row_of = np.zeros(n_new, np.int64)
    row_of[e[:, 5]] = e[:, 0]
    return hop, dict(dst_ptr=ptr.astype(np.int32), src_idx=e[:, 4].astype(np.int32), rel=e[:, 2].astype(np.int32),
                     row_of_dst=row_of.astype(np.int32))


def source_view(A, n_src):
    """The source-segmented view of the destination-ordered arrays ``A``: src_ptr [n_src + 1], edge_of [E] (the stable sort by source)
    and dst_of_edge [E], int32."""
    src = A["src_idx"].astype(np.int64)
    ptr = np.zeros(n_src + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(src, minlength=n_src))
    dst_of = np.repeat(np.arange(len(A["dst_ptr"]) - 1), np.diff(A["dst_ptr"].astype(np.int64)))
    return dict(src_ptr=ptr.astype(np.int32), edge_of=np.argsort(src, kind="stable").astype(np.int32), dst_of_edge=dst_of.astype(np.int32))


def take_sources(A, V, pick):
    """The call that carries only the sources ``pick`` (ascending) of (A, V), renumbered 0 .. len(pick) - 1, with every destination
    and the other tables as they are: (A', V', at) with ``at`` the kept edges' positions in A's list."""
    at = np.nonzero(np.isin(A["src_idx"], pick))[0]
    new_id = np.full(len(V["src_ptr"]) - 1, -1, np.int64)
    new_id[pick] = np.arange(len(pick))
    dst = V["dst_of_edge"][at].astype(np.int64)
    ptr = np.zeros(len(A["dst_ptr"]), np.int64)
    ptr[1:] = np.cumsum(np.bincount(dst, minlength=len(A["dst_ptr"]) - 1))
    A2 = dict(dst_ptr=ptr.astype(np.int32), src_idx=new_id[A["src_idx"][at]].astype(np.int32), rel=A["rel"][at], row_of_dst=A["row_of_dst"])
    return A2, source_view(A2, len(pick)), at


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def case(name, d, ld, attn, ap=None, seed=0, **kw):
    """tests/test_digraph_layer_gpu.py's case: layer_ref's default graph, five queries, two hops."""
    c = lr._case(name, seed=seed, d=d, ld=ld, attn_dim=attn, B=5, **kw)
    if ap is not None:
        c.ap = ap
    return c


ROW_WIDTHS = [(d, ld) for d in (16, 20) for ld in (32, 64, 128, 256)] + [(16, 16), (64, 64)]
ATTENTION_WIDTHS = [(3, 4), (5, 8), (16, 16), (17, 32), (3, 32)]
HUB_DEGREES = (0, 1, 127, 128, 129, 256, 257, 3000)      # 128: the longest source that is not cut; 3000: 24 chunks


def row_width_case(d, ld):
    return case("d%d_ld%d" % (d, ld), d, ld, 5, seed=d + ld)


def attention_case(attn, ap):
    return case("attn%d_ap%d" % (attn, ap), 16, 32, attn, ap=ap, seed=attn + ap)


def hub_hop(n_ones=1000, n_dst=300, B=3, seed=41):
    """A hand-built hop: sources 0..7 of HUB_DEGREES out-edges, then ``n_ones`` sources of one edge each, into ``n_dst`` random
    destinations of ``B`` rows with random relations.  (case, hop, A): layer_ref case and hop, the forward's arrays."""
    c = case("hub_sources", 20, 32, 5, seed=seed, n_rel=3, triples=np.zeros((1, 3), np.int64), nodes0=np.zeros((1, 2), np.int64))
    c.B = B
    rng = np.random.default_rng(seed)
    deg = np.array(HUB_DEGREES + (1,) * n_ones)
    src = np.repeat(np.arange(len(deg)), deg)
    E = len(src)
    dst = rng.integers(0, n_dst, E)
    dst[:n_dst] = rng.permutation(n_dst)                  # every destination has an edge
    order = rng.permutation(E)                            # the list order inside a destination is not the source order
    src, dst = src[order], dst[order]
    row_of = rng.integers(0, B, n_dst)
    edges = np.stack([row_of[dst], src, rng.integers(0, c.n_rela_rows, E), dst, src, dst], 1)
    hop, A = by_destination(edges, len(deg), n_dst)
    return c, hop, A


def one_edge_hop():
    c = case("one_edge", 16, 32, 5, seed=5)
    hop = lr.static_hop(np.array([[1, 7, 2, 9, 3, 0]]), 4, 1)
    A = dict(dst_ptr=np.array([0, 1], np.int32), src_idx=np.array([3], np.int32), rel=np.array([2], np.int32),
             row_of_dst=np.array([1], np.int32))
    return c, hop, A


def case_hops(c):
    """[(k, hop, A)] of a layer_ref case: its oracle hops re-ordered by destination."""
    return [(k,) + by_destination(edges, len(old), len(new)) for k, (old, new, edges, _) in enumerate(lr.hops(c))]


def all_hops():
    """Every (tag, case, k, hop, A) the kernel's tests use."""
    out = []
    for c in [row_width_case(d, ld) for d, ld in ROW_WIDTHS] + [attention_case(a, ap) for a, ap in ATTENTION_WIDTHS]:
        out += [("%s hop %d" % (c.name, k + 1), c, k, hop, A) for k, hop, A in case_hops(c)]
    c, hop, A = hub_hop()
    out.append((c.name, c, 0, hop, A))
    c, hop, A = one_edge_hop()
    out.append((c.name, c, 0, hop, A))
    return out


def tables(x):
    """The reference's positional arguments from layer_ref.inputs' dict."""
    return tuple(x[k] for k in ("hidden", "rela", "a_s", "a_r", "a_q", "w_alpha", "b_alpha", "grad_agg"))
