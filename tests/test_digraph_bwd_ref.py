"""tests/digraph_bwd_ref.py on its own (no GPU): the fp32 run of the reference stays within layer_ref.REF32_WORST_RATIO of the fp64 run
under layer_ref's error model on every hop the kernel's tests use, grad_gate's model included; the gate gradient is the derivative
it claims to be; and the source view and the hub list are what the kernel's tests assume."""
import numpy as np
import pytest

from tests import digraph_bwd_ref as D
from tests import layer_ref as lr

_HOPS = {}


def _hops():
    if not _HOPS:
        _HOPS.update({tag: (c, k, hop, A) for tag, c, k, hop, A in D.all_hops()})
    return _HOPS


def test_fp32_reference_within_its_bound_on_every_case():
    worst = dict.fromkeys(D.OUTPUTS, 0.0)
    for tag, (c, k, hop, A) in _hops().items():
        x = lr.inputs(c, k, hop)
        r64, r32 = D.backward(hop, *D.tables(x)), D.backward(hop, *D.tables(x), dtype=np.float32)
        for name in D.OUTPUTS:
            assert getattr(r32, name).dtype == np.float32
            ratio = lr.worst_ratio(getattr(r32, name), getattr(r64, name), r64.S[name], r64.n[name], D.n0_of(name, c.d, c.attn_dim))
            worst[name] = max(worst[name], ratio)
            assert ratio <= lr.REF32_WORST_RATIO, "%s %s: fp32 reference at ratio %.3g" % (tag, name, ratio)
        print("%s: E %d" % (tag, hop.E))
    print("worst ratios of the fp32 reference: %s (allowed %.3g)" % (worst, lr.REF32_WORST_RATIO))


def test_gate_gradient_is_the_derivative_of_the_gated_forward():
    """d <G, agg> / d g_e by central differences on the fp64 forward with the gate written out; alpha does not see the gate."""
    c, k, hop, A = _hops()["d20_ld32 hop 2"]
    x = {kk: None if v is None else np.asarray(v, np.float64) for kk, v in lr.inputs(c, k, hop).items()}
    _, _, alpha = lr._attention(hop, x["a_s"], x["a_r"], x["a_q"], x["w_alpha"], x["b_alpha"])
    m = lr._message(hop, x["hidden"], x["rela"], None)

    def loss(g):
        return float((x["grad_agg"] * lr._scatter(hop.o, (g * alpha)[:, None] * m, hop.n_new)).sum())
    want = D.backward(hop, *D.tables(x)).grad_gate
    rng = np.random.default_rng(0)
    for e in rng.integers(0, hop.E, 20):
        g = np.ones(hop.E)
        g[e] = 1 + 1e-6
        up = loss(g)
        g[e] = 1 - 1e-6
        assert abs((up - loss(g)) / 2e-6 - want[e]) <= 1e-7 * max(1.0, abs(want[e]))


def test_source_view_is_a_stable_permutation():
    c, k, hop, A = _hops()["hub_sources"]
    V = D.source_view(A, hop.n_old)
    deg = np.diff(V["src_ptr"].astype(np.int64))
    assert deg[:len(D.HUB_DEGREES)].tolist() == list(D.HUB_DEGREES) and (deg[len(D.HUB_DEGREES):] == 1).all() and len(deg) > 1000
    assert np.array_equal(np.sort(V["edge_of"]), np.arange(hop.E))
    for s in range(len(D.HUB_DEGREES)):
        mine = V["edge_of"][V["src_ptr"][s]:V["src_ptr"][s + 1]]
        assert (A["src_idx"][mine] == s).all() and (np.diff(mine) > 0).all()         # the source's edges, in list order
    assert np.array_equal(V["dst_of_edge"], hop.o) and (np.diff(hop.o) >= 0).all()
    # a sub-call keeps the edges' order and renumbers the sources
    pick = np.arange(0, hop.n_old, 3)
    A2, V2, at = D.take_sources(A, V, pick)
    assert np.array_equal(pick[A2["src_idx"]], A["src_idx"][at]) and np.array_equal(V2["dst_of_edge"], V["dst_of_edge"][at])
    assert np.array_equal(np.diff(V2["src_ptr"]), deg[pick])


def test_reference_on_a_typed_in_hop():
    """Two edges into one destination from one source, d = 1, no attention input: alpha = sigmoid(b_alpha)."""
    hop = lr.static_hop(np.array([[0, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0]]), 1, 1)
    hidden, rela = np.array([[2.0]]), np.array([[1.0], [-3.0]])
    zero = np.zeros((1, 4))
    r = D.backward(hop, hidden, rela, zero, np.zeros((2, 4)), zero, np.array([1.0]), np.array([0.0]), np.array([[5.0]]))
    assert np.allclose(r.grad_gate, [0.5 * 5 * 3, 0.5 * 5 * -1]) and np.allclose(r.grad_hidden, [[0.5 * 5 * 2]])
    assert not r.grad_a_s.any()                                                       # relu'(0) = 0
    assert np.allclose(r.S["grad_gate"], [0.5 * 5 * 3, 0.5 * 5 * 5]) and r.n["grad_gate"].tolist() == [1, 1]
